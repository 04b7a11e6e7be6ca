"""Trees whose field is not finite at finite points, and their sample tables -- TEST INFRASTRUCTURE ONLY.
No GPU.

A leaf under a finite, invertible matrix of scale 2^-64 .. 2^-67 sees local coordinates of up to 2^68: they
stay finite, but the primitive's own arithmetic overflows, and the oracle's field is +Inf, -Inf or NaN
(Inf - Inf) over whole regions of the box +-1.  This is not program.hpp's documented limit (a scale chain
that makes a coordinate itself infinite): tests/test_cpu_nonfinite.py asserts that every leaf's local
coordinates stay below 2^100, and what classes of samples every case holds, on the oracle's field alone.
tests/test_gpu_nonfinite.py compares every grid and ray query with its numpy restatement fed with that
field.  A field is computed once per (tree, table) and left unchanged.

  iheart @ 2^-64   NaN for x >= 0.75 and z >= 0.0625, elsewhere +Inf above z = 0.0625 and -Inf below
  icone  @ 2^-66   a finite negative core of radius 0.1 around the axis x = -0.25, y = 0.125; around it -Inf
                   on the planes near its apex (z = 0.0625, 0.3) and NaN on those further away (z = 0.7, -0.3)
  sheared iheart   the same leaf under x' = x - y (XF_GENERIC): its NaN region x - y >= 0.625 cuts a cap
                   off the sphere
The sphere of every tree has radius 1/2 around (0.125, 0, 0).  A CSG select keeps a NaN in one operand
position and drops it in the other (the reference's min and max are a < b ? a : b), so Union(sphere, leaf)
and Union(leaf, sphere) differ wherever the leaf is NaN.
"""
import json

import numpy as np

import np_mass
import np_raster
import np_raycast
import np_slice
import ray_edge_inputs as edges
from implisolid_amd import scenes

f32 = np.float32
EYE = scenes.EYE
LEVELS = [0, 2]
SCALE = 2.0 ** -64
CONE_SCALE = 2.0 ** -66    # between 2^-64 (-Inf, no NaN) and 2^-69 (NaN but for four samples): probed on the oracle
T = (-0.25, 0.125, 0.0625)
LIMIT = 2.0 ** 100


def sheared(scale, a, tx, ty, tz):
    """forward x = s (x' + a y') + tx: the inverse is x' = ((x - tx) - a (y - ty)) / s, exact for a = 1"""
    return [scale, a * scale, 0, tx, 0, scale, 0, ty, 0, 0, scale, tz]


SPHERE = {"type": "iellipsoid", "matrix": scenes.st(1.0, 0.125, 0, 0)}
HEART = {"type": "iheart", "matrix": scenes.st(SCALE, *T)}
CONE = {"type": "icone", "matrix": scenes.st(CONE_SCALE, *T)}
HEART_SHEARED = {"type": "iheart", "matrix": sheared(SCALE, 1.0, *T)}


def node(kind, a, b):
    return {"type": kind, "matrix": list(EYE), "children": [a, b]}


def deep(inner, n=13):
    """inner as the second operand of n nested unions with spheres of radius 0.1 far from the box: the second
    operand is evaluated over the first one's value, so the program depth grows by one a level, and a Union
    keeps its second operand's NaN"""
    t = inner
    for i in range(n):
        t = node("Union", {"type": "iellipsoid", "matrix": scenes.st(0.2, 5.0, 5.0, 5.0 + i)}, t)
    return t


TREES = {
    "inter": node("Intersection", HEART, SPHERE),
    "union_sl": node("Union", SPHERE, HEART),
    "union_ls": node("Union", HEART, SPHERE),
    "diff": node("Difference", SPHERE, HEART),
    "cone": node("Union", SPHERE, CONE),
    "shear": node("Intersection", HEART_SHEARED, SPHERE),
}
TREES["deep"] = deep(TREES["shear"])
NAMES = sorted(TREES)
# the classes of samples a case claims on every table (asserted in test_cpu_nonfinite.py, 100 of each):
# "nan", "pinf", "ninf", "neg" (finite and < 0), "pos" (finite and not < 0)
CLAIMS = {
    "inter": {"nan", "neg", "pos"},
    "union_sl": {"nan", "pinf"},             # a Union with +Inf has no finite sample above z = 0.0625
    "union_ls": {"pinf", "neg"},             # the sphere's value where the leaf is NaN
    "diff": {"nan", "ninf"},
    "cone": {"nan", "neg", "pos"},
    "shear": {"nan", "neg", "pos"},
    "deep": {"nan", "neg", "pos"},
}
MIXED = [n for n in NAMES if {"nan", "neg", "pos"} <= CLAIMS[n]]   # the cases with a NaN region beside a real surface
ORDER_PAIR = ("union_sl", "union_ls")


def classes(F):
    """name -> bool mask of the samples of that class"""
    F = np.asarray(F, f32)
    fin = np.isfinite(F)
    with np.errstate(invalid="ignore"):
        return {"nan": np.isnan(F), "pinf": F == np.inf, "ninf": F == -np.inf, "neg": fin & (F < 0), "pos": fin & ~(F < 0)}


def leaves_local(shape, pts):
    """[(leaf type, float64 (n, 3) local coordinates of pts)] through the inverses of the matrices on the path,
    each inverted in float64"""
    def inv(m):
        A = np.eye(4)
        A[:3, :] = np.array(m[:12], np.float64).reshape(3, 4)
        return np.linalg.inv(A)

    def walk(n, P):
        A = inv(n["matrix"])
        Q = P @ A[:3, :3].T + A[:3, 3]
        if "children" in n:
            return [x for c in n["children"] for x in walk(c, Q)]
        return [(n["type"], Q)]
    return walk(shape, np.asarray(pts, np.float64).reshape(-1, 3))


# ---- the fields ------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
        if isinstance(_CACHE[key], np.ndarray):
            _CACHE[key].setflags(write=False)
    return _CACHE[key]


def tree_of(oracle, name):
    return _cached(("tree", name), lambda: oracle.mp5_to_nodes(json.dumps(TREES[name])))


def field(oracle, name, key, pts):
    """the oracle's field of TREES[name] at pts, once per (name, key)"""
    return _cached(("F", name, key), lambda: np.asarray(oracle.eval_implicit(tree_of(oracle, name), np.ascontiguousarray(pts, f32)), f32))


# ---- the grid tables ----------------------------------------------------------------------------------------------
RECT = [-1.0, 1.0, -1.0, 1.0]
BOX = [-1.0, 1.0, -1.0, 1.0, -1.0, 1.0]
GRIDS = [(40, 40, 2), (33, 17, 4)]    # W, H, s: tiles of 16, 16, 8 pixels; border tiles one pixel wide and high
SLICE_R = [40, 33]
DEPTHS = [5, 6]
# above and below the leaves' plane z = 0.0625 and on it, a plane above the sphere (z > 1/2: only what the leaf
# makes solid), and 0.3 over -0.3 over 0.3: a layer of one side of the plane rests on one of the other side
Z = np.array([0.3, 0.7, 0.3, -0.3, 0.3, 0.0625, -0.55], f32)
TILE = 16


def raster_table(W, H, s):
    mx, my = np_raster.coords(RECT, W, H, s)
    return mx, my, np_raster.points(mx, my, Z)


def raster_field(oracle, name, W, H, s):
    """F (L, H s, W s)"""
    return field(oracle, name, ("raster", W, H, s), raster_table(W, H, s)[2]).reshape(len(Z), H * s, W * s)


def raster_tiles(W, H, s):
    """[(l, y sample slice, x sample slice, box)] of the (layer, 16 x 16-pixel tile) pairs: the box the raster
    kernel bounds is the one of the tile's end samples and {z, z}"""
    mx, my, _ = raster_table(W, H, s)
    out = []
    for l, z in enumerate(Z):
        for ty in range((H + TILE - 1) // TILE):
            for tx in range((W + TILE - 1) // TILE):
                i0, i1 = s * TILE * tx, s * min(TILE * tx + TILE, W)
                j0, j1 = s * TILE * ty, s * min(TILE * ty + TILE, H)
                out.append((l, slice(j0, j1), slice(i0, i1), [mx[i0], mx[i1 - 1], my[j0], my[j1 - 1], z, z]))
    return out


def slice_table(R):
    xs, ys = np_slice.coords(np.array(RECT, f32), R)
    return xs, ys, np_slice.points(xs, ys, Z)


def slice_field(oracle, name, R):
    """F (L, R + 1, R + 1)"""
    return field(oracle, name, ("slice", R), slice_table(R)[2]).reshape(len(Z), R + 1, R + 1)


def slice_tiles(R):
    """as raster_tiles for the slicer's tiles of 16 x 16 cells: the samples 16 t .. min(16 t + 16, R), both ends"""
    xs, ys, _ = slice_table(R)
    nt = (R + TILE - 1) // TILE
    out = []
    for l, z in enumerate(Z):
        for ty in range(nt):
            for tx in range(nt):
                i0, i1 = TILE * tx, min(TILE * tx + TILE, R)
                j0, j1 = TILE * ty, min(TILE * ty + TILE, R)
                out.append((l, slice(j0, j1 + 1), slice(i0, i1 + 1), [xs[i0], xs[i1], ys[j0], ys[j1], z, z]))
    return out


def mass_field(oracle, name, depth):
    """F (N, N, N) indexed [k][j][i]"""
    N = 1 << depth
    return field(oracle, name, ("mass", depth), np_mass.points(np_mass.mids(BOX, depth))).reshape(N, N, N)


def mass_boxes(depth):
    """[(z, y, x cell slices, box)] of the boxes of the levels 3 .. depth of the mass descent: the box of level
    v and index (ix, iy, iz) spans the edges i << (depth - v) and (i + 1) << (depth - v)"""
    import np_bounds
    E = np_bounds.edges(BOX, depth)
    out = []
    for level in range(3, depth + 1):
        sh = depth - level
        n = 1 << level
        for iz in range(n):
            for iy in range(n):
                for ix in range(n):
                    a = [(i << sh, (i + 1) << sh) for i in (ix, iy, iz)]
                    out.append((slice(*a[2]), slice(*a[1]), slice(*a[0]),
                                [E[0][a[0][0]], E[0][a[0][1]], E[1][a[1][0]], E[1][a[1][1]], E[2][a[2][0]], E[2][a[2][1]]]))
    return out


def box_classes(F, items):
    """per item of raster_tiles / slice_tiles / mass_boxes (any_solid, any_outside) of the samples it holds"""
    with np.errstate(invalid="ignore"):
        neg = np.asarray(F) < 0
    out = np.empty((len(items), 2), bool)
    for n, it in enumerate(items):
        sub = neg[it[0], it[1], it[2]]
        out[n] = [(~sub).any(), sub.any()]
    return out


# ---- the rays --------------------------------------------------------------------------------------------------------
RAY_N = [130, 4200]
ROUNDS = [0, 24]


CORE_X0 = [-0.4, -0.38, -0.36, -0.3]
CORE_T = 1.25


def core_rays():
    """rays that start in the icone's finite core (|x + 0.25| < 0.25 on the plane y = 0.125), outside the sphere,
    and leave it through x = -0.5 at t = 1.25, still outside the sphere: the field is finite and < 0 up to there
    and NaN from there on.  Of N = 130 the first segment (t <= 0.985) lies in the core"""
    o = np.array([[x0, 0.125, -0.9] for x0 in CORE_X0], f32)
    d = np.array([[-(x0 + 0.5) / CORE_T, 0, 0.5] for x0 in CORE_X0], f32)
    return o, d


def _grid_rays():
    """rays across the box at z = 0.3 and z = 0.7 along +x and -x (rows of different y), along +z and -z through
    the leaves' plane, and oblique ones in the planes y = const and across all three axes"""
    o, d = [], []
    for y in np.linspace(-0.9, 0.9, 13):
        for z in (0.3, 0.7):
            o += [[-1.0, y, z], [1.0, y, z]]
            d += [[1, 0, 0], [-1, 0, 0]]
    for x in np.linspace(-0.45, 0.95, 15):
        for y in (-0.3, 0.125, 0.45):
            o += [[x, y, -1.0], [x, y, 1.0]]
            d += [[0, 0, 1], [0, 0, -1]]
    for y in np.linspace(-0.6, 0.6, 7):
        for sx in (1, -1):
            o += [[-0.9 * sx, y, -0.8], [-0.9 * sx, y, 0.9], [0.9 * sx, -y, 0.6]]
            d += [[0.9 * sx, 0, 0.8], [0.9 * sx, 0.1, -0.5], [-0.9 * sx, 0.35, -0.45]]
    # from z = 0.2, where every tree but for the iheart's NaN region is finite or infinite, up and down into the
    # planes on which the icone's field is NaN: brackets from a sample < 0 onto a NaN one outside the sphere
    for x in (-0.8, -0.6, 0.9):
        for y in (-0.7, 0.6):
            o += [[x, y, 0.2], [x, y, 0.2]]
            d += [[0, 0, 1], [0, 0, -1]]
    o2, d2 = core_rays()
    return np.array(o + o2.tolist(), f32), np.array(d + d2.tolist(), f32)


def ray_case(name, N):
    """the rays of _grid_rays with t in [0, 2]: every sample point is finite (asserted here)"""
    def make():
        o, d = _grid_rays()
        c = edges.Case(("nonfinite", name, N), TREES[name], o, d, 0.0, 2.0, N)
        T = np.broadcast_to(c.ts[None, :], (len(c), len(c.ts)))
        assert np.isfinite(np_raycast.points(c.o, c.d, T)).all() and np.isfinite(c.o).all() and np.isfinite(c.d).all()
        return c
    return _cached(("rays", name, N), make)


# a NaN entry in the march kernel's second batch (samples beyond 4096 of N = 4200).  "inter": along +x from x = -1
# the leaf's NaN region starts at x = 0.75, t = 1.75 of t1 = 1.78.  "cone": core_rays, which enter the NaN region at
# t = 1.25 of t1 = 1.27 through segments the bound can prove outside (the icone's bound is finite in its core)
LATE = {"inter": 1.78, "cone": 1.27}
LATE_NAMES = sorted(LATE)


def late_case(name):
    def make():
        if name == "cone":
            o, d = core_rays()
        else:
            ys = np.linspace(-0.9, 0.9, 7)
            o = np.array([[-1.0, y, 0.3] for y in ys], f32)
            d = np.tile(np.array([1, 0, 0], f32), (len(o), 1))
        return edges.Case(("nonfinite_late", name), TREES[name], o, d, 0.0, LATE[name], 4200)
    return _cached(("late", name), make)


def ray_field(oracle, case):
    """F (n, N + 1), the oracle's"""
    return edges.sampled(oracle, case)
