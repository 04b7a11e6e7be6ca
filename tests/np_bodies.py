"""numpy restatement of the bodies of the layer stack -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_layer_bodies), independent of the kernels:

  target     a voxel (l, py, px) is of the target class iff (cov[l][py][px] >= threshold) == (target == 1)
  adjacent   two target voxels that differ by one step in exactly one of px, py, l (connectivity 6), or by at
             most one step in each and are not equal (connectivity 26); inside the stack only
  body       a class of the transitive closure of adjacency; its seed is its smallest key l W H + py W + px
  record     int64 {seed, volume, x0, y0, l0, x1, y1, l1}: the voxel count and the inclusive bounding box;
             the records come in increasing seed
  row run    a maximal sequence of target voxels within one image row: int32 {start = py W + x0, length, body},
             body the index of its body's record; layer by layer in increasing start, run_offsets (L + 1,)

Bodies by minimum-key propagation in 3D, as np_islands.labels does in 2D: every target voxel starts with its
own key and takes the smallest key among itself and its target neighbours until nothing changes.
"""
import itertools

import numpy as np

FIELDS = ("seed", "volume", "x0", "y0", "l0", "x1", "y1", "l1")
RUN_FIELDS = ("start", "length", "body")
STEPS26 = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]   # (dl, dy, dx)
STEPS6 = [d for d in STEPS26 if sum(abs(v) for v in d) == 1]


def steps(connectivity):
    assert connectivity in (6, 26)
    return STEPS6 if connectivity == 6 else STEPS26


def labels(mask, connectivity):
    """mask bool (L, H, W) -> int64 (L, H, W): the smallest key of the voxel's body, -1 where the mask is off"""
    mask = np.asarray(mask, bool)
    L, H, W = mask.shape
    big = L * H * W
    lab = np.where(mask, np.arange(big, dtype=np.int64).reshape(L, H, W), big)
    st = steps(connectivity)
    while True:
        p = np.pad(lab, 1, constant_values=big)
        m = lab
        for dl, dy, dx in st:
            m = np.minimum(m, p[1 + dl:1 + dl + L, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        m = np.where(mask, m, big)
        if np.array_equal(m, lab):
            break
        lab = m
    return np.where(mask, lab, -1)


def records(lab):
    """int64 (B, 8) of a labelled stack, in increasing seed"""
    L, H, W = lab.shape
    ll, py, px = np.nonzero(lab >= 0)
    seeds, inv = np.unique(lab[ll, py, px], return_inverse=True)
    rec = np.zeros((len(seeds), 8), np.int64)
    rec[:, 0] = seeds
    rec[:, 1] = np.bincount(inv, minlength=len(seeds))
    for col, v in ((2, px), (3, py), (4, ll)):
        lo = np.full(len(seeds), np.iinfo(np.int64).max)
        hi = np.full(len(seeds), -1, np.int64)
        np.minimum.at(lo, inv, v)
        np.maximum.at(hi, inv, v)
        rec[:, col], rec[:, col + 3] = lo, hi
    return rec


def row_runs(lab, rec):
    """(run_offsets int64 (L + 1,), runs int32 (R, 3)) of a labelled stack and its records"""
    L, H, W = lab.shape
    on = lab >= 0
    before = np.zeros_like(on)
    before[:, :, 1:] = on[:, :, :-1]
    after = np.zeros_like(on)
    after[:, :, :-1] = on[:, :, 1:]
    sl, sy, sx = np.nonzero(on & ~before)     # row-major: layer by layer, row by row, left to right
    el, ey, ex = np.nonzero(on & ~after)      # the k-th end closes the k-th start
    assert np.array_equal(sl, el) and np.array_equal(sy, ey) and (ex >= sx).all()
    runs = np.stack([sy * W + sx, ex - sx + 1, np.searchsorted(rec[:, 0], lab[sl, sy, sx])], axis=1).astype(np.int32)
    offs = np.concatenate(([0], np.cumsum(np.bincount(sl, minlength=L)))).astype(np.int64)
    return offs, runs.reshape(-1, 3)


def bodies(cov, threshold, target, connectivity):
    """cov uint8 (L, H, W) -> (run_offsets, records int64 (B, 8), runs int32 (R, 3), decode int32 (L, H, W) = the
    voxel's body index or -1)"""
    assert target in (0, 1)
    mask = (np.asarray(cov) >= threshold) == (target == 1)
    lab = labels(mask, connectivity)
    rec = records(lab)
    offs, runs = row_runs(lab, rec)
    decode = np.where(mask, np.searchsorted(rec[:, 0], lab), -1).astype(np.int32)
    return offs, rec, runs, decode


def as_rows(a, fields=FIELDS):
    """a structured record array (implisolid_amd.BODY_DTYPE or BODY_RUN_DTYPE) as integers (n, fields)"""
    a = np.asarray(a)
    if a.dtype.names:
        assert a.dtype.names == fields
        return np.stack([a[n] for n in fields], axis=1).reshape(-1, len(fields))
    return a.reshape(-1, len(fields))
