"""NumPy restatement of the hollowing query -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_layer_hollow, implisolid_hollow_wall2) by brute
force, independent of the kernels and of any distance transform: a solid voxel is core unless an empty voxel
lies in its lens, and the lens is searched directly -- every offset (dy, dx) with dy^2 + dx^2 <= wall2[|j|] of
every layer l + j within reach is looked at, in the image's pixels only.  A layer outside the stack on a side
whose bit of `ends` is set is searched as an all-empty layer; with the bit clear it does not exist.
"""
import math

import numpy as np

FIELDS = ("solid", "core")
MAX_REACH = 1024


def wall2_table(wall, pitch):
    """implisolid_hollow_wall2 in Python floats (doubles; every product and the difference rounded on its own);
    None where the entry refuses"""
    wall, pitch = float(wall), float(pitch)
    if not math.isfinite(wall) or wall < 0 or not math.isfinite(pitch) or pitch <= 0:
        return None
    w2 = wall * wall
    if not w2 < 2.0 ** 30:
        return None
    out = []
    j = 0
    while True:
        h = float(j) * pitch
        hh = h * h
        if not hh <= w2:
            break
        if j > MAX_REACH:
            return None
        out.append(int(math.floor(w2 - hh)))
        j += 1
    return out


def offsets(r2, H, W):
    """the disc's offsets (dy, dx) that can join two pixels of an H x W image"""
    r = math.isqrt(int(r2))
    return [(dy, dx) for dy in range(-min(r, H - 1), min(r, H - 1) + 1) for dx in range(-min(r, W - 1), min(r, W - 1) + 1)
            if dy * dy + dx * dx <= r2]


def reached(empty, r2):
    """(H, W) bool: the pixels p with an empty pixel q of the layer at |q - p|^2 <= r2"""
    H, W = empty.shape
    hit = np.zeros((H, W), bool)
    for dy, dx in offsets(r2, H, W):   # q = p + (dy, dx)
        ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
        xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
        hit[yd, xd] |= empty[ys, xs]
    return hit


def core(solid, wall2, ends):
    """(L, H, W) bool: the core voxels of the solid mask"""
    solid = np.asarray(solid, bool)
    L, H, W = solid.shape
    wall2 = [int(v) for v in wall2]
    reach = len(wall2) - 1
    assert reach >= 0 and all(0 <= v < 1 << 30 for v in wall2) and all(a >= b for a, b in zip(wall2, wall2[1:])) and ends in (0, 1, 2, 3)
    nothing = np.ones((H, W), bool)   # a virtual layer: every pixel empty
    cache = {}

    def hit(m, r2):
        if m < 0 or m >= L:
            if not ends & (1 if m < 0 else 2):
                return None
            key = ("virtual", r2)
            layer = nothing
        else:
            key = (m, r2)
            layer = ~solid[m]
        if key not in cache:
            cache[key] = reached(layer, r2)
        return cache[key]

    out = solid.copy()
    for l in range(L):
        for j in range(-reach, reach + 1):
            h = hit(l + j, wall2[abs(j)])
            if h is not None:
                out[l] &= ~h
    return out


def hollow(cov, threshold, wall2, ends):
    """(out uint8 (L, H, W), records int64 (L, 2) = {solid, core}) of a coverage stack"""
    cov = np.asarray(cov, np.uint8)
    solid = cov >= threshold
    c = core(solid, wall2, ends)
    out = np.where(c, np.uint8(0), cov).astype(np.uint8)
    rec = np.stack([solid.sum(axis=(1, 2)), c.sum(axis=(1, 2))], axis=1).astype(np.int64)
    return out, rec


def as_rows(records):
    """a structured records array as int64 (L, 2)"""
    r = np.asarray(records)
    return np.stack([r[name] for name in FIELDS], axis=1).astype(np.int64)
