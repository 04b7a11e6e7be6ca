"""numpy restatement of the run-length layer images -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_layer_runs), independent of the kernels that
compute it:

  inputs   cov uint8 (L, H, W), implisolid_raster's coverage; threshold
  values   threshold == 0: v = cov; threshold >= 1: v = (cov >= threshold) as 0 / 1
  stream   layer l is v[l] read row by row: p = py W + px, p in [0, W H)
  runs     a run starts at p = 0 and at every p > 0 with v[p] != v[p - 1]; per run its start (uint32) and its
           value (uint8), in increasing start; run_offsets int64 (L + 1,) delimits the layers
  lengths  the next start of the layer minus the run's own, W H - start for a layer's last run

The coverage is an argument.
"""
import numpy as np


def values(cov, threshold):
    cov = np.asarray(cov, np.uint8)
    return cov if threshold == 0 else (cov >= threshold).astype(np.uint8)


def encode(cov, threshold):
    """(run_offsets int64 (L + 1,), start uint32 (R,), value uint8 (R,))"""
    v = values(cov, threshold)
    L = v.shape[0]
    flat = v.reshape(L, -1)
    offs, starts, vals = [0], [], []
    for l in range(L):
        first = np.ones(flat.shape[1], bool)
        first[1:] = flat[l, 1:] != flat[l, :-1]
        at = np.flatnonzero(first)
        starts.append(at.astype(np.uint32))
        vals.append(flat[l, at])
        offs.append(offs[-1] + len(at))
    return np.array(offs, np.int64), np.concatenate(starts), np.concatenate(vals).astype(np.uint8)


def lengths(run_offsets, start, layer_pixels):
    """int64 (R,)"""
    out = np.empty(len(start), np.int64)
    for l in range(len(run_offsets) - 1):
        a, b = int(run_offsets[l]), int(run_offsets[l + 1])
        ends = np.append(np.asarray(start[a + 1:b], np.int64), layer_pixels)
        out[a:b] = ends - np.asarray(start[a:b], np.int64)
    return out


def decode(run_offsets, start, value, W, H):
    """uint8 (L, H, W)"""
    n = lengths(run_offsets, start, W * H)
    return np.repeat(np.asarray(value, np.uint8), n).reshape(len(run_offsets) - 1, H, W)
