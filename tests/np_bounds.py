"""numpy restatement of the bounds of a solid -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_bounds), independent of the kernels that
compute it: the float32 edge table, the float64 fitted-box formula, and the plain descent with no
skipping, driven level by level through implisolid_amd.debug_intervals (the interval probe, which is
older than the bounds pass and tested box by box in test_gpu_intervals.py).  One numpy ufunc call is
one IEEE operation.
"""
import numpy as np

f32 = np.float32


def edges(search, depth):
    """float32 [3, N + 1]: edge[k] = lo + (float)k * ((hi - lo) / (float)N), edge[N] = hi."""
    s = np.asarray(search, np.float32).reshape(3, 2)
    N = 1 << depth
    k = np.arange(N, dtype=np.float32)
    out = np.empty((3, N + 1), np.float32)
    for a in range(3):
        lo, hi = s[a]
        step = np.divide(np.subtract(hi, lo, dtype=np.float32), f32(N), dtype=np.float32)
        out[a, :N] = np.add(lo, np.multiply(k, step, dtype=np.float32), dtype=np.float32)
        out[a, N] = hi
    return out


def fit_box(search, bounds, resolution, margin):
    """float32 [6], or None where the formula has no cells left (resolution - 2 margin < 1)."""
    if margin < 0 or resolution - 2 * margin < 1:
        return None
    s = np.asarray(search, np.float32).astype(np.float64).reshape(3, 2)
    b = np.asarray(bounds, np.float32).astype(np.float64).reshape(3, 2)
    out = np.empty((3, 2), np.float64)
    for a in range(3):
        w = (b[a, 1] - b[a, 0]) / np.float64(resolution - 2 * margin)
        out[a, 0] = max(s[a, 0], b[a, 0] - np.float64(margin) * w)
        out[a, 1] = min(s[a, 1], b[a, 1] + np.float64(margin) * w)
    return out.astype(np.float32).reshape(6)


def classify(iv):
    """0 mixed, 1 solid (lo >= 0), 2 outside (hi < 0): brick_modes.hpp sign_class; a NaN bound is mixed."""
    lo, hi = iv[:, 0], iv[:, 1]
    solid = lo >= 0
    outside = ~solid & (hi < 0)
    return np.where(solid, 1, np.where(outside, 2, 0))


def descent(impli, shape, search, depth, ignore_root_matrix=False):
    """The definition, level by level with no skipping.  Returns (found, box float32[6], info) with
    info = dict(evaluated=boxes bounded, listed=[mixed boxes per level 3 .. depth])."""
    E = edges(search, depth)
    g = np.arange(8, dtype=np.int64)
    idx = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)   # (x, y, z) of level 3
    modes = np.zeros(len(idx), np.uint64)
    lo = np.full(3, np.inf, np.float32)
    hi = np.full(3, -np.inf, np.float32)
    evaluated, listed = 0, []
    oct_ = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij"), axis=-1).reshape(-1, 3)
    for level in range(3, depth + 1):
        if len(idx) == 0:
            listed.append(0)
            continue
        sh = depth - level
        b0 = np.stack([E[a][idx[:, a] << sh] for a in range(3)], axis=1)
        b1 = np.stack([E[a][(idx[:, a] + 1) << sh] for a in range(3)], axis=1)
        boxes = np.stack([b0[:, 0], b1[:, 0], b0[:, 1], b1[:, 1], b0[:, 2], b1[:, 2]], axis=1)
        iv, mo = impli.debug_intervals(shape, boxes, variant=0, modes_in=modes, ignore_root_matrix=ignore_root_matrix)
        evaluated += len(idx)
        c = classify(iv)
        give = (c == 1) | ((c == 0) & (level == depth))
        if give.any():
            lo = np.minimum(lo, b0[give].min(axis=0))
            hi = np.maximum(hi, b1[give].max(axis=0))
        cut = (c == 0) & (level < depth)
        listed.append(int((c == 0).sum()))
        idx = (2 * idx[cut][:, None, :] + oct_[None, :, :]).reshape(-1, 3)
        modes = np.repeat(mo[cut], 8)
    found = bool(np.isfinite(lo).all())
    s = np.asarray(search, np.float32)
    box = np.stack([lo, hi], axis=1).reshape(6).astype(np.float32) if found else s.copy()
    return found, box, {"evaluated": evaluated, "listed": listed}
