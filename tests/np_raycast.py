"""numpy restatement of the ray cast against a solid -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_raycast, implisolid_ray_params),
independent of the kernels that compute it:

  params    ts[k] = t0 + (float)k * ((t1 - t0) / (float)N) for k < N, ts[N] = t1
  points    p(t) = o + t * d, the product and the sum rounded to float32 on their own
  solid     not (F < 0): -0.0 and NaN are solid
  per ray   k = the smallest index in 0 .. N with a solid sample
            none: hit -1, t = t1, f = 0;  k = 0: hit 0, t = ts[0], f = F(ts[0])
            k >= 1: hit k; a = ts[k - 1], b = ts[k], fb = F(b); B rounds of m = a + 0.5f * (b - a),
            fm = F(m), solid -> b = m, fb = fm, else a = m; t = b, f = fb

The field is an argument: field_fn(points float32 (m, 3)) -> float32 (m,).  cast() evaluates all N + 1
samples of all rays at once and then runs B vectorised rounds with one field_fn call each, over every
ray (rows without a bracket are evaluated at a harmless point and ignored).  One numpy ufunc call is
one IEEE operation.
"""
import numpy as np

f32 = np.float32


def params(t0, t1, N):
    """N + 1 float32 sample parameters"""
    t0, t1 = f32(t0), f32(t1)
    with np.errstate(all="ignore"):
        step = np.divide(np.subtract(t1, t0, dtype=f32), f32(N), dtype=f32)
        ts = np.empty(N + 1, f32)
        off = np.multiply(np.arange(N, dtype=f32), step, dtype=f32)
        ts[:N] = np.add(t0, off, dtype=f32)
    ts[N] = t1
    return ts


def points(o, d, t):
    """p(t) float32: o, d (n, 3); t (n,) gives (n, 3), t (n, m) gives (n, m, 3)"""
    o = np.asarray(o, f32).reshape(-1, 3)
    d = np.asarray(d, f32).reshape(-1, 3)
    t = np.asarray(t, f32)
    if t.ndim == 2:
        o, d = o[:, None, :], d[:, None, :]
    with np.errstate(all="ignore"):
        return np.add(o, np.multiply(t[..., None], d, dtype=f32), dtype=f32)


def sample_field(field_fn, o, d, ts):
    """F float32 (n, N + 1) at every sample of every ray"""
    n = np.asarray(o).reshape(-1, 3).shape[0]
    T = np.broadcast_to(np.asarray(ts, f32)[None, :], (n, len(ts)))
    return np.asarray(field_fn(np.ascontiguousarray(points(o, d, T).reshape(-1, 3))), f32).reshape(n, len(ts))


def cast(field_fn, o, d, ts, B, F=None):
    """(hit int32 (n,), t float32 (n,), f float32 (n,)); F: sample_field's values, when the caller keeps them"""
    ts = np.asarray(ts, f32)
    N = len(ts) - 1
    if F is None:
        F = sample_field(field_fn, o, d, ts)
    with np.errstate(invalid="ignore"):
        solid = ~(F < 0)
    any_solid = solid.any(axis=1)
    k = np.where(any_solid, solid.argmax(axis=1), -1).astype(np.int32)
    rows = np.arange(len(k))
    t = np.where(k >= 0, ts[np.maximum(k, 0)], ts[N]).astype(f32)
    f = np.where(k >= 0, F[rows, np.maximum(k, 0)], f32(0)).astype(f32)
    br = k >= 1                                   # rows with a bracket
    a = ts[np.maximum(k - 1, 0)].astype(f32)
    b = t.copy()
    for _ in range(B):
        half = np.multiply(f32(0.5), np.subtract(b, a, dtype=f32), dtype=f32)
        m = np.add(a, half, dtype=f32)
        fm = np.asarray(field_fn(np.ascontiguousarray(points(o, d, m))), f32)
        with np.errstate(invalid="ignore"):
            sm = ~(fm < 0)
        up = br & sm
        b = np.where(up, m, b)
        f = np.where(up, fm, f)
        a = np.where(br & ~sm, m, a)
    return k, np.where(br, b, t).astype(f32), f.astype(f32)
