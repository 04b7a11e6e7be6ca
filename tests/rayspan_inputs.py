"""Inputs and references of the span tests -- TEST INFRASTRUCTURE ONLY.  No GPU (but for the sdf_3d shape,
whose field comes from ImplicitService as in tests/test_gpu_raycast.py).

tests/test_gpu_rayspans.py compares implisolid_ray_spans with np_rayspans.spans of the oracle's field on the
rays built here; tests/test_cpu_rayspans.py asserts on the oracle's field alone what the GPU tests rely on
(which rays hold 0, 1 and more spans, where the placed entries and exits fall), so an edit that spoils an
input fails without a GPU.  A sampled field is computed once per (case, N) and a reference once per (case,
N, B); both are left unchanged.
"""
import numpy as np

import np_raycast
import np_rayspans
import test_gpu_mass as gm
import test_gpu_raycast as tg
from implisolid_amd import scenes

f32 = np.float32
EYE = scenes.EYE
SEG = 64
SPHERE, BIG, AWAY = gm.SPHERE, gm.BIG, gm.AWAY
# two spheres of radius 1/4 at z = +-1/2; the sphere of radius 1/2 with a cavity of radius 1/4
TWO = {"type": "Union", "matrix": EYE, "children": [{"type": "iellipsoid", "matrix": scenes.st(0.5, 0, 0, 0.5)},
                                                   {"type": "iellipsoid", "matrix": scenes.st(0.5, 0, 0, -0.5)}]}
SHELL = {"type": "Difference", "matrix": EYE, "children": [SPHERE, {"type": "iellipsoid", "matrix": scenes.st(0.5, 0, 0, 0)}]}
SHAPES = dict(gm.SHAPES, two=TWO, shell=SHELL)
NAMES = sorted(SHAPES)
INSIDE = {"two": [0, 0, 0.5], "shell": [0.375, 0, 0]}
# shapes a line can enter twice (asserted in tests/test_cpu_rayspans.py on the oracle's field); an ellipsoid
# (egg, the sdf_3d sphere) holds at most one span a ray whatever the rays are
SEVERAL = ["csg", "shell", "tree_deep", "twist", "two"]
T0 = tg.T0
# behind test_gpu_raycast's 257 rays: down and up the z axis through both spheres of TWO and the cavity of
# SHELL, along x through the cavity, and a zero direction at the hollow centre
EXTRA_O = np.array([[0, 0, 2], [0, 0, -2], [-2, 0, 0], [0, 0, 0]], f32)
EXTRA_D = np.array([[0, 0, -1], [0, 0, 1.5], [1, 0, 0], [0, 0, 0]], f32)
N_RAYS = tg.N_RAYS + len(EXTRA_O)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def nseg(N):
    return (N + SEG - 1) // SEG


def case(impli, oracle, name):
    """(o, d, t1, field_fn): test_gpu_raycast's rays of the shape and the extra ones; t1 lies just behind
    the entry of the axis-parallel ray 1, which therefore ends inside at every N"""
    def make():
        if name in gm.SHAPES:
            o, d, t1, fn = tg._case(impli, oracle, name)
        else:
            fn = tg._field_fn(impli, oracle, name, SHAPES[name])
            o, d = tg._rays(INSIDE[name])
            fine = np_raycast.cast(fn, o[1:2], d[1:2], np_raycast.params(T0, 4.25, 4000), 24)
            assert fine[0][0] >= 1
            t1 = float(f32(fine[1][0] + 0.004))
        return np.concatenate([o, EXTRA_O]), np.concatenate([d, EXTRA_D]), t1, fn
    return _cached(("case", name), make)


class Rays:
    """One shape, its rays and its sample table (ray_edge_inputs.Case's fields)."""

    def __init__(self, key, shape, o, d, t0, t1, N):
        self.key, self.shape, self.t0, self.t1, self.N = key, shape, t0, t1, N
        self.o = np.ascontiguousarray(o, f32).reshape(-1, 3)
        self.d = np.ascontiguousarray(d, f32).reshape(-1, 3)
        self.ts = np_raycast.params(t0, t1, N)

    def __len__(self):
        return len(self.o)

    def args(self, B):
        return self.shape, self.o, self.d, self.t0, self.t1, self.N, B


def suite(impli, oracle, name, N):
    o, d, t1, _ = case(impli, oracle, name)
    return _cached(("suite", name, N), lambda: Rays(("suite", name, N), SHAPES[name], o, d, T0, t1, N))


def reference(impli, oracle, rays, B, name="oracle", normals=True, ignore_root_matrix=False):
    """(offsets, k, t, f, normals (S, 2, 3)) of np_rayspans.spans on a field that does not come from the ray
    kernels (test_gpu_raycast._field_fn's sources), and np_normals' normals at the ends"""
    fn = tg._field_fn(impli, oracle, name, rays.shape, ignore_root_matrix)
    F = _cached(("F", rays.key, name), lambda: np_raycast.sample_field(fn, rays.o, rays.d, rays.ts))

    def make():
        offs, k, t, f = np_rayspans.spans(fn, rays.o, rays.d, rays.ts, B, F=F)
        nrm = np.zeros((len(k), 2, 3), f32)
        if normals and len(k):
            pts = np_rayspans.end_points(rays.o, rays.d, offs, t).reshape(-1, 3)
            nrm = np.asarray(tg._normals_at(impli, oracle, name, rays.shape, pts, ignore_root_matrix), f32).reshape(-1, 2, 3)
        return offs, k, t, f, nrm
    return _cached(("ref", rays.key, name, B, normals), make)


# ---- entries and exits on chosen samples --------------------------------------------------------------------
# N = 4200: 66 segments, so the second batch holds two; the last segment is partial (40 samples)
PLACED_N, PLACED_T0, PLACED_T1 = 4200, 0.25, 4.25
PLACED_KS = [64, 65, 4096, 4097, PLACED_N]
ACROSS_K = 4150   # an exit there: the span holds the samples 4096 and 4097, the two sides of the batch boundary


def placed_case(which):
    """Rays down the z axis from (0, 0, z0) with a pole midway between the samples K - 1 and K (raycast-edges'
    trick).  "sphere": the top pole (an entry at K), then the bottom pole (an exit at K) for every K of
    PLACED_KS, then an exit at ACROSS_K.  "two": the far sphere's top pole (its entry at K), then its bottom
    pole (its exit at K)."""
    def make():
        ts = np_raycast.params(PLACED_T0, PLACED_T1, PLACED_N).astype(np.float64)
        mid = lambda K: (ts[K - 1] + ts[K]) / 2   # noqa: E731
        top, bottom = (0.5, -0.5) if which == "sphere" else (-0.25, -0.75)
        z0 = [top + mid(K) for K in PLACED_KS] + [bottom + mid(K) for K in PLACED_KS]
        if which == "sphere":
            z0.append(bottom + mid(ACROSS_K))
        o = np.zeros((len(z0), 3))
        o[:, 2] = z0
        d = np.tile([0.0, 0, -1], (len(o), 1))
        return Rays(("placed", which), SPHERE if which == "sphere" else TWO, o, d, PLACED_T0, PLACED_T1, PLACED_N)
    return _cached(("placed", which), make)


def zero_rays():
    """test_gpu_raycast's -0.0 case: the 1024 node lines in x of gm.zero_node(), N = 31, every sample a node"""
    def make():
        node, zeros = gm.zero_node()
        nodes = (f32(-0.96875) + f32(0.0625) * np.arange(32, dtype=f32)).astype(f32)
        zz, yy = np.meshgrid(nodes, nodes, indexing="ij")
        o = np.stack([np.full(1024, nodes[0], f32), yy.reshape(-1), zz.reshape(-1)], -1).astype(f32)
        d = np.tile(np.array([1, 0, 0], f32), (1024, 1))
        return Rays("zero", node, o, d, 0.0, 1.9375, 31), zeros
    return _cached("zero", make)
