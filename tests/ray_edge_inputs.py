"""Inputs and references of the ray caster's edge tests -- TEST INFRASTRUCTURE ONLY.  No GPU.

tests/test_gpu_raycast_edges.py compares implisolid_raycast with np_raycast.cast of the oracle's field on
the rays built here; tests/test_cpu_raycast.py asserts that these inputs still hold what the GPU tests
rely on (hits on chosen samples of every batch, hits beyond sample 4096 and misses, a ray that passes
one solid and hits another, overflowed sample points whose field is NaN, hits on both sides of t = 0),
so an edit that spoils them fails without a GPU.  The field values come from the oracle, never from the
ray kernels.  The sampled field is computed once per case and a reference once per (case, B); both are
left unchanged.

A ray's segment j holds the samples 64 j + 1 .. 64 j + 64 (segment 0 sample 0 as well); the march
kernel bounds 64 segments a batch, so a second batch starts at sample 4097.
"""
import numpy as np

import np_raycast
import test_gpu_mass as gm
from implisolid_amd import scenes
from test_gpu_raycast import _field_fn, _normals_at

f32 = np.float32
EYE = scenes.EYE
SEG = 64
LEVELS = [0, 2]


def nseg(N):
    return (N + SEG - 1) // SEG


class Case:
    """One shape, its rays and its sample table."""

    def __init__(self, key, shape, o, d, t0, t1, N):
        self.key, self.shape, self.t0, self.t1, self.N = key, shape, t0, t1, N
        self.o = np.ascontiguousarray(o, f32).reshape(-1, 3)
        self.d = np.ascontiguousarray(d, f32).reshape(-1, 3)
        self.ts = np_raycast.params(t0, t1, N)

    def __len__(self):
        return len(self.o)

    def args(self, B):
        return self.shape, self.o, self.d, self.t0, self.t1, self.N, B


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def sampled(oracle, case, impli=None, source="oracle"):
    """F (n, N + 1): the field at every sample of every ray, once per case"""
    fn = _field_fn(impli, oracle, source, case.shape)
    return _cached(("F", case.key, source), lambda: np_raycast.sample_field(fn, case.o, case.d, case.ts))


def reference(oracle, case, B, impli=None, source="oracle", normals=True):
    """(hit, t, f, normals) of np_raycast.cast on the field of `source`: "oracle", or "sdf3d" for
    ImplicitService.eval and .normals (test_gpu_raycast._field_fn's names); normals=False leaves them zero"""
    def make():
        fn = _field_fn(impli, oracle, source, case.shape)
        hit, t, f = np_raycast.cast(fn, case.o, case.d, case.ts, B, F=sampled(oracle, case, impli, source))
        nrm = np.zeros((len(case), 3), f32)
        rows = hit >= 0
        if normals:
            nrm[rows] = _normals_at(impli, oracle, source, case.shape, np_raycast.points(case.o, case.d, t)[rows])
        return hit, t, f, nrm
    return _cached(("ref", case.key, source, B, normals), make)


def segment_boxes(case):
    """(n, nseg, 6) float32 {xlo, xhi, ylo, yhi, zlo, zhi}: per ray and segment j the box the march kernel
    bounds, whose per-axis ends are the ordered coordinates of p(ts[64 j]) and p(ts[min(64 j + 64, N)])
    (a < b ? {a, b} : {b, a}, as the kernel orders them)"""
    k0 = SEG * np.arange(nseg(case.N))
    k1 = np.minimum(k0 + SEG, case.N)
    n = len(case)
    a = np_raycast.points(case.o, case.d, np.broadcast_to(case.ts[k0], (n, len(k0))))
    b = np_raycast.points(case.o, case.d, np.broadcast_to(case.ts[k1], (n, len(k0))))
    less = a < b
    lo, hi = np.where(less, a, b), np.where(less, b, a)
    return np.stack([lo[..., 0], hi[..., 0], lo[..., 1], hi[..., 1], lo[..., 2], hi[..., 2]], -1).astype(f32)


def hit_segment(rh, N):
    """per ray the last segment the walk reaches: the hit's, segment 0 for a ray that starts inside, the
    last one on a miss"""
    rh = np.asarray(rh)
    return np.where(rh < 0, nseg(N) - 1, np.maximum(rh - 1, 0) // SEG)


def expected_work(hi, rh, N):
    """(skipped, evaluated) summed over the rays, from the upper bounds hi (n, nseg) of segment_boxes:
    of the segments up to the hit segment those proved outside (hi < 0) are skipped, the others
    evaluated; no hit segment may be proved outside"""
    jh = hit_segment(rh, N)
    upto = np.arange(nseg(N))[None, :] <= jh[:, None]
    with np.errstate(invalid="ignore"):
        out = hi < 0
    rows = np.flatnonzero(np.asarray(rh) >= 0)
    assert not out[rows, jh[rows]].any(), "a segment that holds a solid sample is never proved outside"
    return int((out & upto).sum()), int((~out & upto).sum())


# ---- 1. hits on chosen samples, across batches -----------------------------------------------------------
T0, T1 = 0.25, 4.25
PLACED_N = [4097, 8200, 65536]
MISSES = 2   # the last rays of a placed case


def placed_ks(N):
    """both sides of segment boundaries in the first, second and third batch, and the last samples"""
    ks = [1, 63, 64, 65, 127, 128, 129, 4032, 4033, 4095, 4096, 4097, 4098, 4159, 4160, 4161, 8191, 8192, 8193, N - 1, N]
    return np.array(sorted(set(k for k in ks if k <= N)), np.int32)


def placed_case(N):
    """the sphere of radius 1/2 and rays down the z axis whose first solid sample is placed_ks(N)[i]: the
    sphere's pole lies midway between samples K - 1 and K; then a ray that misses and a zero direction
    outside"""
    def make():
        ts = np_raycast.params(T0, T1, N).astype(np.float64)
        ks = placed_ks(N)
        o = np.zeros((len(ks) + MISSES, 3))
        o[:len(ks), 2] = 0.5 + (ts[ks - 1] + ts[ks]) / 2
        d = np.tile([0.0, 0, -1], (len(o), 1))
        o[-2], d[-2] = [2, 2, 2], [1, 0, 0]
        o[-1], d[-1] = [1.5, 1.5, 1.5], [0, 0, 0]
        return Case(("placed", N), gm.SPHERE, o, d, T0, T1, N)
    return _cached(("placed", N), make)


SEEDED_N = 8200
SEEDED_NAMES = ["csg", "tree_deep"]
SEEDED_RAYS = 64
# name -> a point inside the solid (asserted in tests/test_cpu_raycast.py)
SEEDED_INSIDE = {"csg": [-0.2, 0.0, 0.1], "tree_deep": [0.3, -0.1, 0.2]}


def seeded_case(name):
    """64 rays from the sphere of radius 2: three of four aimed near SEEDED_INSIDE[name], the others at
    points of the box +-0.75; every second direction of length 0.45, so that its hits lie beyond half
    the range (sample 4096 and the second batch)"""
    def make():
        rng = np.random.default_rng(17)
        n = SEEDED_RAYS
        v = rng.normal(size=(n, 3))
        o = 2.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
        target = rng.uniform(-0.75, 0.75, size=(n, 3))
        near = np.arange(n) % 4 != 3
        target[near] = np.asarray(SEEDED_INSIDE[name], np.float64) + rng.uniform(-0.15, 0.15, size=(int(near.sum()), 3))
        d = target - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d[0::2] *= 0.45
        return Case(("seeded", name), gm.SHAPES[name], o, d, T0, T1, SEEDED_N)
    return _cached(("seeded", name), make)


# ---- 3. a gap between a live segment and the hit ---------------------------------------------------------------
# radius 1/4 at z = 1 and radius 1/2 at z = -1.5
TWO_SPHERES = {"type": "Union", "matrix": EYE, "children": [{"type": "iellipsoid", "matrix": scenes.st(0.5, 0, 0, 1.0)},
                                                           {"type": "iellipsoid", "matrix": scenes.st(1.0, 0, 0, -1.5)}]}
GAP_X = [0.0, 0.26, 0.3, 0.4, 0.6]
GAP_HITS = [2460, 6270, 6315, 6479, -1, 6326]
GAP_N = 8200
GAP_PASS = 1      # the ray at x = 0.26 passes the small sphere at a field value of -0.082
GAP_OBLIQUE = 5   # passes the small sphere's centre at a distance of 0.2515, 11.5 degrees off the z axis
OBLIQUE_O, OBLIQUE_D = [0.66484725, 0.0, 3.0], [-0.2, 0.0, -0.98]
GAP_RANGES = {"unit": (1.0, 0.25, 5.25),       # the directions' factor, t0, t1
              "halved": (0.5, 0.5, 10.5),      # d halved, t0 and t1 doubled: ts doubles exactly, the same points
              "halved_t1": (0.5, 0.25, 10.5)}  # d halved, t1 alone doubled: from z = 2.875, a step 1.025 times as long


def gap_case(which="unit"):
    """rays down z from (x, 0, 3) and the oblique ray, in one of GAP_RANGES.  The box of a segment of an
    axis-parallel ray is the segment itself, which the bound follows to within its margin: only the
    oblique ray's boxes reach into the small sphere while none of its samples does"""
    def make():
        factor, t0, t1 = GAP_RANGES[which]
        o = np.array([[x, 0, 3] for x in GAP_X] + [OBLIQUE_O], f32)
        d = np.array([[0, 0, -1]] * len(GAP_X) + [OBLIQUE_D], f32) * f32(factor)
        return Case(("gap", which), TWO_SPHERES, o, d, t0, t1, GAP_N)
    return _cached(("gap", which), make)


def gap_chunk_case():
    """ten rays of the gap case (x from 0 to 0.63): four chunks of three, the last of one ray"""
    def make():
        o = np.array([[0.07 * i, 0, 3] for i in range(10)], f32)
        d = np.tile(np.array([0, 0, -1], f32), (10, 1))
        return Case("gap_chunks", TWO_SPHERES, o, d, 0.25, 5.25, GAP_N)
    return _cached("gap_chunks", make)


# ---- 4. overflowed sample points ---------------------------------------------------------------------------------
OVERFLOW_T1 = 3e38
OVERFLOW_N = [130, 4200]
OVERFLOW_NAMES = ["egg", "csg"]
OVERFLOW_INSIDE = {"egg": [0.25, 0.5, -0.3], "csg": [0.25, 0.5, -0.5]}
# of length about 4, every component non-zero, one negative, the components of different sizes so that
# they overflow at different samples
OVERFLOW_DIRS = [[2.5, -2.0, 2.375], [-1.5, 3.0, 2.25], [2.3, 2.2, -2.3], [3.5, -1.0, 1.75]]


def overflow_case(name, N):
    """rays that leave the solid's neighbourhood for good: t0 = 0, t1 = 3e38, so ts[k] * d overflows from
    some sample on.  Then a ray that starts inside and a zero direction outside."""
    def make():
        p = np.asarray(OVERFLOW_INSIDE[name], np.float64)
        dirs = np.asarray(OVERFLOW_DIRS, np.float64)
        o = np.concatenate([p + 0.25 * dirs, [p, [1.5, 1.5, 1.5]]])
        d = np.concatenate([dirs, [dirs[0], [0, 0, 0]]])
        return Case(("overflow", name, N), gm.SHAPES[name], o, d, 0.0, OVERFLOW_T1, N)
    return _cached(("overflow", name, N), make)


def first_overflowed(case):
    """per ray the first sample with a coordinate that is not finite, -1 where there is none"""
    T = np.broadcast_to(case.ts[None, :], (len(case), len(case.ts)))
    bad = ~np.isfinite(np_raycast.points(case.o, case.d, T)).all(axis=2)
    return np.where(bad.any(axis=1), bad.argmax(axis=1), -1)


# ---- 5. small cases ---------------------------------------------------------------------------------------------
BEHIND_T0, BEHIND_T1, BEHIND_N = -1.5, 2.5, 130


def behind_case(o, d):
    """the suite's rays (test_gpu_raycast._rays of twist's inside point) with every origin moved 1.5
    parameter units along its direction: the samples with t < 0 lie where the suite's rays start"""
    def make():
        o2 = (np.asarray(o, np.float64) + 1.5 * np.asarray(d, np.float64)).astype(f32)
        return Case("behind", gm.SHAPES["twist"], o2, d, BEHIND_T0, BEHIND_T1, BEHIND_N)
    return _cached("behind", make)
