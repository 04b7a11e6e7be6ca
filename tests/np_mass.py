"""numpy / Python-int restatement of the mass properties of a solid -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_mass, implisolid_mass_mids,
implisolid_mass_physical), independent of the kernels: the float32 sample table, the ten integer
moments and the layer counts of a field array passed in, and the physical conversion with Python ints
for the exact part.  One numpy ufunc call is one IEEE operation.
"""
import numpy as np

import np_bounds

f32 = np.float32


def mids(box, depth):
    """float32 [3, N]: mid[k] = edge[k] + 0.5f * (edge[k + 1] - edge[k]) over np_bounds.edges."""
    E = np_bounds.edges(box, depth)
    w = np.subtract(E[:, 1:], E[:, :-1], dtype=np.float32)
    half = np.multiply(f32(0.5), w, dtype=np.float32)
    return np.add(E[:, :-1], half, dtype=np.float32)


def points(M):
    """float32 [N^3, 3], x fastest then y then z: the sample points of a mids table."""
    z, y, x = np.meshgrid(M[2], M[1], M[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3), np.float32)


def solid(F):
    """marching cubes' rule: solid iff !(F < 0); -0.0 and NaN are solid."""
    return ~(np.asarray(F, np.float32) < 0)


def moments_of_cells(i, j, k):
    """Ten Python ints from the solid cells' index arrays."""
    i, j, k = ([int(v) for v in a] for a in (i, j, k))
    s = lambda a, b=None: sum(a) if b is None else sum(p * q for p, q in zip(a, b))   # noqa: E731
    return [len(i), s(i), s(j), s(k), s(i, i), s(j, j), s(k, k), s(i, j), s(j, k), s(i, k)]


def moments(F):
    """(ten Python ints, layer_cells int64 [N]) of a field F [N, N, N] indexed [k][j][i]."""
    S = solid(F)
    N = S.shape[0]
    assert S.shape == (N, N, N)
    k, j, i = np.nonzero(S)
    # exact in int64 for N <= 2^10 (the largest sum is below 2^49); returned as Python ints
    i, j, k = i.astype(np.int64), j.astype(np.int64), k.astype(np.int64)
    m = [len(i), i.sum(), j.sum(), k.sum(), (i * i).sum(), (j * j).sum(), (k * k).sum(), (i * j).sum(), (j * k).sum(),
         (i * k).sum()]
    return [int(v) for v in m], S.reshape(N, -1).sum(axis=1).astype(np.int64)


def _s1(a, b):
    return sum(range(a, b))


def _s2(a, b):
    return sum(v * v for v in range(a, b))


def box_moments(i0, i1, j0, j1, k0, k1):
    """Ten Python ints of the full index range [i0, i1) x [j0, j1) x [k0, k1)."""
    ni, nj, nk = i1 - i0, j1 - j0, k1 - k0
    return [ni * nj * nk, nj * nk * _s1(i0, i1), ni * nk * _s1(j0, j1), ni * nj * _s1(k0, k1),
            nj * nk * _s2(i0, i1), ni * nk * _s2(j0, j1), ni * nj * _s2(k0, k1),
            nk * _s1(i0, i1) * _s1(j0, j1), ni * _s1(j0, j1) * _s1(k0, k1), nj * _s1(i0, i1) * _s1(k0, k1)]


def physical(box, depth, m):
    """(empty, float64 [10] = [volume, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Iyz, Ixz]) from ten ints."""
    m = [int(v) for v in m]
    b = np.asarray(box, np.float32).astype(np.float64).reshape(3, 2)
    N = np.float64(1 << depth)
    d = [(b[a, 1] - b[a, 0]) / N for a in range(3)]
    out = np.zeros(10, np.float64)
    n = m[0]
    if n == 0:
        return True, out
    nd = np.float64(n)                       # n <= 2^30: exact
    cell = (d[0] * d[1]) * d[2]
    volume = nd * cell
    out[0] = volume
    for a in range(3):
        out[1 + a] = b[a, 0] + (np.float64(m[1 + a]) / nd + np.float64(0.5)) * d[a]

    def mu(a, c, sab):
        cab = n * sab - m[1 + a] * m[1 + c]                     # exact
        q = np.float64(float(cab)) / (nd * nd)                  # float(int) rounds to nearest, once
        if a == c:
            q = q + np.float64(1.0) / np.float64(12.0)
        else:
            q = q + np.float64(0.0)
        return ((volume * d[a]) * d[c]) * q
    mxx, myy, mzz = mu(0, 0, m[4]), mu(1, 1, m[5]), mu(2, 2, m[6])
    mxy, myz, mxz = mu(0, 1, m[7]), mu(1, 2, m[8]), mu(0, 2, m[9])
    out[4:] = [myy + mzz, mxx + mzz, mxx + myy, -mxy, -myz, -mxz]
    return False, out


def cuboid_sum(box, depth, i, j, k):
    """An independent float64 route: (volume, centre [3], inertia about the centre [3, 3]) of the cells
    as cuboids -- second moments about the origin summed cell by cell, then the parallel-axis shift."""
    b = np.asarray(box, np.float32).astype(np.float64).reshape(3, 2)
    N = float(1 << depth)
    d = (b[:, 1] - b[:, 0]) / N
    idx = np.stack([np.asarray(i), np.asarray(j), np.asarray(k)], axis=1).astype(np.float64)
    c = b[:, 0][None, :] + (idx + 0.5) * d[None, :]            # cell centres
    cell = d[0] * d[1] * d[2]
    V = cell * len(c)
    com = c.mean(axis=0)
    I0 = np.zeros((3, 3))
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        I0[a, a] = ((c[:, u] ** 2 + c[:, v] ** 2) * cell).sum() + len(c) * cell * (d[u] ** 2 + d[v] ** 2) / 12.0
        I0[a, u] = I0[u, a] = -(c[:, a] * c[:, u] * cell).sum()
    r2 = (com ** 2).sum()
    return V, com, I0 - V * (r2 * np.eye(3) - np.outer(com, com))
