"""numpy restatement of the pixel distance field of the layers -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_layer_distance) by brute force, independent of
the kernels:

  solid        a pixel of layer l is solid iff cov[l][py][px] >= threshold, cov being np_raster.coverage's
  D2(p)        the minimum of (px - qx)^2 + (py - qy)^2 over the pixels q of the same layer whose solidity
               differs from p's; NONE = 2^30 where there is no such pixel.  Only the image's pixels exist
  dist         int32 (L, H, W): +D2 for a solid pixel, -D2 for an empty one
  record       {solid, widest, widest_at, unsupported} per layer, int64: the solid pixels, the largest D2 over
               them (0 without any), the smallest py W + px that attains it (-1 without any), and for l >= 1
               the solid pixels whose pixel in layer l - 1 has dist < -reach2 (0 for l = 0)

Every pixel against every pixel of the other class, in int64, a block of pixels at a time.
"""
import numpy as np

FIELDS = ("solid", "widest", "widest_at", "unsupported")
NONE = 1 << 30
BLOCK = 256


def _mins(py, px, qy, qx):
    out = np.empty(len(py), np.int64)
    for i in range(0, len(py), BLOCK):
        dy = py[i:i + BLOCK, None] - qy[None, :]
        dx = px[i:i + BLOCK, None] - qx[None, :]
        out[i:i + BLOCK] = (dy * dy + dx * dx).min(axis=1)
    return out


def layer_d2(solid):
    """solid bool (H, W) -> signed int64 (H, W)"""
    solid = np.asarray(solid, bool)
    sy, sx = (a.astype(np.int64) for a in np.nonzero(solid))
    ey, ex = (a.astype(np.int64) for a in np.nonzero(~solid))
    d2 = np.full(solid.shape, NONE, np.int64)
    if len(sy) and len(ey):
        d2[sy, sx] = _mins(sy, sx, ey, ex)
        d2[ey, ex] = _mins(ey, ex, sy, sx)
    return np.where(solid, d2, -d2)


def field(solid):
    """solid bool (L, H, W) -> dist int32 (L, H, W)"""
    return np.stack([layer_d2(s) for s in np.asarray(solid, bool)]).astype(np.int32)


def records(dist, reach2):
    """dist (L, H, W) -> int64 (L, 4)"""
    dist = np.asarray(dist, np.int64)
    L = dist.shape[0]
    rows = np.zeros((L, 4), np.int64)
    for l in range(L):
        flat = dist[l].reshape(-1)
        solid = flat > 0
        rows[l, 0] = solid.sum()
        rows[l, 1] = flat[solid].max() if solid.any() else 0
        rows[l, 2] = int(np.argmax(np.where(solid, flat, 0))) if solid.any() else -1   # the first of the largest
        if l >= 1:
            rows[l, 3] = (solid & (dist[l - 1].reshape(-1) < -int(reach2))).sum()
    return rows


def distance(cov, threshold, reach2):
    """cov uint8 (L, H, W) -> (dist int32 (L, H, W), records int64 (L, 4))"""
    dist = field(np.asarray(cov) >= threshold)
    return dist, records(dist, reach2)


def as_rows(rec):
    """a structured record array (implisolid_amd.DIST_DTYPE) as int64 (L, 4)"""
    rec = np.asarray(rec)
    if rec.dtype.names:
        assert rec.dtype.names == FIELDS
        return np.stack([rec[n] for n in FIELDS], axis=1).astype(np.int64).reshape(-1, 4)
    return rec.astype(np.int64).reshape(-1, 4)
