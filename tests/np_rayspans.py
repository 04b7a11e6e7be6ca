"""numpy restatement of the solid spans along rays -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_ray_spans), independent of the kernels that
compute it.  The sample table, the points and the sampled field are np_raycast's:

  solid     s[k] = not (F(ts[k]) < 0), k = 0 .. N: -0.0 and NaN are solid
  span      a maximal run of solid samples k_in .. k_out - 1; k_out = N + 1: the ray ends inside
  entry     k_in = 0: t = ts[0], f = F(ts[0]); else a = ts[k_in - 1], b = ts[k_in], fb = F(b), B rounds of
            m = a + 0.5f * (b - a), fm = F(m), solid -> b = m, fb = fm, else a = m; t = b, f = fb
  exit      k_out = N + 1: t = ts[N], f = F(ts[N]); else a = ts[k_out - 1], fa = F(a), b = ts[k_out], the
            same rounds with solid -> a = m, fa = fm, else b = m; t = a, f = fa
  a round with m == a or m == b ends that end's rounds

The field is an argument: field_fn(points float32 (m, 3)) -> float32 (m,).  spans() evaluates all N + 1
samples of all rays at once, finds the runs with one difference along the rays, and refines all entries and
all exits together in B vectorised rounds of one field_fn call each (ends without a bracket are evaluated
at a harmless point and ignored).  One numpy ufunc call is one IEEE operation.
"""
import numpy as np

import np_raycast

f32 = np.float32


def runs(solid):
    """(rows, k_in, k_out): the maximal runs of True along axis 1 of solid (n, N + 1), rays in order and a
    ray's runs in increasing k_in"""
    n = solid.shape[0]
    pad = np.zeros((n, solid.shape[1] + 2), np.int8)
    pad[:, 1:-1] = solid
    step = pad[:, 1:] - pad[:, :-1]                 # step[:, j] = s[j] - s[j - 1], nothing solid outside 0 .. N
    rows, k_in = np.nonzero(step == 1)
    rows_out, k_out = np.nonzero(step == -1)
    assert np.array_equal(rows, rows_out) and (k_in < k_out).all()
    return rows, k_in.astype(np.int32), k_out.astype(np.int32)


def _refine(field_fn, o, d, a, b, f, bracket, solid_is_b, B):
    """B rounds on the brackets [a, b]; f: the field at the solid end.  Returns (t, f) of the solid end"""
    a, b, f = a.copy(), b.copy(), f.copy()
    done = ~bracket
    for _ in range(B):
        half = np.multiply(f32(0.5), np.subtract(b, a, dtype=f32), dtype=f32)
        m = np.add(a, half, dtype=f32)
        done = done | (m == a) | (m == b)
        fm = np.asarray(field_fn(np.ascontiguousarray(np_raycast.points(o, d, m))), f32)
        with np.errstate(invalid="ignore"):
            sm = ~(fm < 0)
        act = ~done
        to_solid_end = act & sm
        if solid_is_b:
            b = np.where(to_solid_end, m, b)
            a = np.where(act & ~sm, m, a)
        else:
            a = np.where(to_solid_end, m, a)
            b = np.where(act & ~sm, m, b)
        f = np.where(to_solid_end, fm, f)
    return (b if solid_is_b else a).astype(f32), f.astype(f32)


def spans(field_fn, o, d, ts, B, F=None):
    """(offsets int64 (n + 1,), k int32 (S, 2), t float32 (S, 2), f float32 (S, 2)); F: np_raycast.sample_field's
    values, when the caller keeps them"""
    o = np.asarray(o, f32).reshape(-1, 3)
    d = np.asarray(d, f32).reshape(-1, 3)
    ts = np.asarray(ts, f32)
    N = len(ts) - 1
    if F is None:
        F = np_raycast.sample_field(field_fn, o, d, ts)
    with np.errstate(invalid="ignore"):
        solid = ~(F < 0)
    rows, k_in, k_out = runs(solid)
    offsets = np.zeros(len(o) + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=len(o)), out=offsets[1:])
    oo, dd = o[rows], d[rows]
    # entries: the solid end is b = ts[k_in]
    t_in, f_in = _refine(field_fn, oo, dd, ts[np.maximum(k_in - 1, 0)], ts[k_in], F[rows, k_in], k_in >= 1, True, B)
    # exits: the solid end is a = ts[k_out - 1]
    t_out, f_out = _refine(field_fn, oo, dd, ts[k_out - 1], ts[np.minimum(k_out, N)], F[rows, k_out - 1], k_out <= N, False, B)
    return offsets, np.stack([k_in, k_out], 1).astype(np.int32), np.stack([t_in, t_out], 1), np.stack([f_in, f_out], 1)


def end_points(o, d, offsets, t):
    """p(t) float32 (S, 2, 3) of the spans' ends"""
    o = np.asarray(o, f32).reshape(-1, 3)
    d = np.asarray(d, f32).reshape(-1, 3)
    rows = np.repeat(np.arange(len(o)), np.diff(offsets))
    return np_raycast.points(o[rows], d[rows], np.asarray(t, f32).reshape(-1, 2))
