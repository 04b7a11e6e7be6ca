"""The interval evaluator (ifunc_interval.hpp eval_iv, jit.cpp tree_iv) tested directly, box by box,
through implisolid_debug_intervals / implisolid_debug_eval_modes.

Ground truth: the CPU oracle's f at 64 float32 points inside each box (the 27-point lattice of
corners, edge midpoints, face centres and centre, plus 37 seeded random points clipped into the box).

  P1 containment   lo <= f(p) <= hi at every sampled point (oracle NaNs left out, at most 0.1 %)
  P2 decisions     the pruned point interpreter under the box's modes gives the oracle's f(p) bit for
                   bit: every skipped select would have returned the kept operand
  P3 nesting       along a chain of nested boxes, the parent's modes as the child's modes_in: P1, P2
  P4 variants      the JIT shape module and the baked module: same modes, endpoints equal under ==
                   (only the sign of a zero endpoint may differ, jit.cpp xform_iv_row)
  P5 point boxes   under the identity, primitives whose interval code mirrors the point code: the
                   bound is the value widened only by settle
  P6 pruning power per tree: true mixed interior bricks <= bricks classed mixed <= the recorded count
                   (tests/golden/prune_power.json, tests/golden/make_prune_power.py)

A bound that is sound but useless ([-inf, inf] for every box) passes P1-P4 and fails P5 and P6.
"""
import json
import os

import numpy as np
import pytest

import matrices
import np_restate
from test_gpu_matrices import OBJECTS

pytestmark = pytest.mark.gpu

H = 2.0 / 32
F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prune_power.json")


# ---- trees ----------------------------------------------------------------------------------------
def _trees():
    from implisolid_amd import scenes
    t = {}
    for i, kind in enumerate(matrices.LEAF_TYPES):
        t["eye_" + kind] = matrices.leaf(kind, matrices.EYE)
        t["rot_" + kind] = matrices.family_leaf(kind, "rot", i)
    t["union_sphere_cube"] = scenes.union_sphere_cube()
    t["config3_tree"] = scenes.config3_tree()
    tw = scenes.twist(0.8, 0.2, -0.1, 0.05, pitch=-0.3)
    t["twist_union"] = {"type": "Union", "matrix": scenes.EYE, "children": [tw, scenes.twist(0.5, 0.3, 0.2, 0.1, pitch=0.3)]}
    t["twist_rot_tree"] = OBJECTS["rot"]
    for seed in (40, 42, 45, 46):
        t["random_%d" % seed] = matrices.random_matrix_tree(seed)
    return t


TREES = _trees()
CSG_TREES = [n for n in sorted(TREES) if not n.startswith(("eye_", "rot_"))]
# P5: interval code that mirrors the point code operation for operation (ifunc_interval.hpp)
MIRRORING = ["iellipsoid", "icylinder", "icone", "iheart", "itorus", "implicit_double_mushroom", "top_bottom_lid",
             "half_plane", "tetrahedron", "meta_balls", "extrusion"]
# named exceptions: {type: reason read in the source}
P5_EXCEPTIONS = {}


# ---- geometry helpers -------------------------------------------------------------------------------
def _leaves_world(shape, M=None):
    """(leaf dict, forward 4x4 float64 from the leaf's local frame to world) for every leaf."""
    m = shape["matrix"]
    A = np.eye(4)
    A[:3, :] = np.array(m[:12], np.float64).reshape(3, 4)
    W = A if M is None else M @ A
    if "children" in shape:
        out = []
        for c in shape["children"]:
            out += _leaves_world(c, W)
        return out
    return [(shape, W)]


def _singular_points(kind, rng, n):
    """Local points on the primitive's singular set: the axis of the screw, cone and cylinder, the
    torus centre circle, the double mushroom's cap planes z = +-0.45, the lid planes z = +-0.5, the
    rabbit table's faces; the centre for the rest."""
    u = rng.uniform(-0.6, 0.6, size=(n, 3))
    if kind in ("screw", "inf_screw", "screw_gradient_wrong", "screw_diff_two_plane", "icone", "icylinder"):
        p = np.zeros((n, 3))
        p[:, 2] = u[:, 2]
        if kind.startswith(("screw", "inf_screw")):
            p[n // 2:, :2] = u[n // 2:, :2]
            p[n // 2:, 2] = rng.choice([-0.5, 0.5], n - n // 2)         # the twist's lid planes
        return p
    if kind == "itorus":
        a = rng.uniform(0, 2 * np.pi, n)
        return np.stack([0.8 * np.cos(a), 0.8 * np.sin(a), np.zeros(n)], 1)
    if kind == "implicit_double_mushroom":
        u[:, 2] = rng.choice([-0.45, 0.45], n)
        return u
    if kind in ("top_bottom_lid", "extrusion"):
        u[:, 2] = rng.choice([-0.5, 0.5], n)
        return u
    if kind == "cube":
        gs = float(np_restate.RCONST["GRID_SIZE"])
        o = [float(np_restate.RCONST["ORIGIN_" + a]) for a in "XYZ"]
        size = [22, 18, 22]
        p = np.stack([rng.uniform(o[a], o[a] + gs * size[a], n) for a in range(3)], 1)
        ax = rng.integers(0, 3, n)
        side = rng.integers(0, 2, n)
        for k in range(n):
            p[k, ax[k]] = o[ax[k]] + gs * size[ax[k]] * side[k]
        return p
    return np.zeros((n, 3))


def _ulp_boxes(centres, rng):
    """Boxes 1 to 16 ulps wide per axis around float32 centres."""
    c = np.ascontiguousarray(centres, np.float32)
    lo = c.copy()
    hi = c.copy()
    steps = rng.integers(1, 17, size=c.shape)
    for _ in range(16):
        m = steps > 0
        hi = np.where(m, np.nextafter(hi, F32(np.inf)), hi)
        steps = steps - 1
    return np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1], lo[:, 2], hi[:, 2]], 1).astype(np.float32)


def _sized_boxes(origin, size):
    o = np.ascontiguousarray(origin, np.float32)
    hi = (o + np.asarray(size, np.float32)).astype(np.float32)
    return np.stack([o[:, 0], hi[:, 0], o[:, 1], hi[:, 1], o[:, 2], hi[:, 2]], 1)


def _box_points(boxes, seed):
    """64 float32 points per box, every one inside it: the 3 x 3 x 3 lattice, then 37 random ones."""
    b = np.ascontiguousarray(boxes, np.float32)
    n = b.shape[0]
    lo, hi = b[:, 0::2], b[:, 1::2]                                   # [n, 3]
    mid = np.clip((lo.astype(np.float64) + hi.astype(np.float64)) / 2, lo, hi).astype(np.float32)
    lat = np.stack([lo, mid, hi], 1)                                  # [n, 3 (pos), 3 (axis)]
    idx = np.array([(i, j, k) for i in range(3) for j in range(3) for k in range(3)])
    p27 = np.stack([lat[:, idx[:, 0], 0], lat[:, idx[:, 1], 1], lat[:, idx[:, 2], 2]], 2)   # [n, 27, 3]
    rng = np.random.default_rng(seed)
    u = rng.random((n, 37, 3))
    pr = (lo[:, None, :].astype(np.float64) + u * (hi.astype(np.float64) - lo.astype(np.float64))[:, None, :]).astype(np.float32)
    pr = np.clip(pr, lo[:, None, :], hi[:, None, :])
    return np.concatenate([p27, pr], 1)                               # [n, 64, 3]


def _root_operands_close(oracle, shape, tree, pts):
    """Among pts, those where the root CSG node's two operands are nearly equal (the operands'
    values from the oracle's own sub-trees at the root's local points; only used to choose inputs)."""
    nodes, root = tree
    c0, c1 = nodes[root].child[0], nodes[root].child[1]
    if c0 < 0 or c1 < 0:
        return pts[:0]
    mi = np.array(nodes[root].minv[:], np.float64).reshape(3, 4)
    loc = (pts.astype(np.float64) @ mi[:, :3].T + mi[:, 3]).astype(np.float32)
    f1, f2 = oracle.eval_implicit((nodes, c0), loc), oracle.eval_implicit((nodes, c1), loc)
    d = np.abs(np.abs(f1) - np.abs(f2))
    d[~np.isfinite(d)] = np.inf
    return pts[np.argsort(d)[:96]]


def _make_boxes(oracle, name):
    """About 2048 world-space boxes of the kinds the passes produce and the kinds that hurt, with the
    kind of each.  Deterministic per tree name."""
    shape = TREES[name]
    tree = oracle.mp5_to_nodes(json.dumps(shape))
    rng = np.random.default_rng(sum(map(ord, name)))
    out, kinds = [], []

    def add(b, kind):
        out.append(np.ascontiguousarray(b, np.float32))
        kinds.extend([kind] * len(b))

    # brick-shaped boxes, origins not grid-aligned: the brick, the flat layer, the coarse box
    for kind, sz, n in (("brick", (7 * H, 7 * H, H), 420), ("flat", (7 * H, 7 * H, 0.0), 300), ("coarse", (7 * H, 7 * H, 15 * H), 300)):
        add(_sized_boxes(rng.uniform(-1.2, 1.2 - max(sz), size=(n, 3)), sz), kind)
    # near-surface points: the samples of smallest |f|
    cand = rng.uniform(-1.2, 1.2, size=(60000, 3)).astype(np.float32)
    fc = np.abs(oracle.eval_implicit(tree, cand))
    fc[~np.isfinite(fc)] = np.inf
    near = cand[np.argsort(fc)[:160]]
    # point boxes
    pb = np.concatenate([cand[:120], near[:80]])
    add(np.repeat(pb, 2, axis=1), "point")
    # tiny boxes at near-surface points and where the root's operands are nearly equal
    add(_ulp_boxes(near, rng), "tiny")
    close = _root_operands_close(oracle, shape, tree, cand)
    if len(close):
        add(_ulp_boxes(close, rng), "tiny")
        add(_sized_boxes(close - F32(H / 2), (H, H, H)), "brick")
    # boxes straddling each primitive's singular set, through the forward matrices
    for lf, W in _leaves_world(shape):
        loc = _singular_points(lf["type"], rng, 36)
        w = (loc @ W[:3, :3].T + W[:3, 3]).astype(np.float32)
        add(_ulp_boxes(w[:12], rng), "singular")
        half = rng.choice([H / 4, H / 2, 3.5 * H], size=(24, 1)).astype(np.float32)
        o = (w[12:] - half * rng.uniform(0.2, 0.8, size=(24, 3)).astype(np.float32)).astype(np.float32)
        hi = (o + 2 * half * np.ones((1, 3), np.float32)).astype(np.float32)
        add(np.stack([o[:, 0], hi[:, 0], o[:, 1], hi[:, 1], o[:, 2], hi[:, 2]], 1), "singular")
    # far boxes
    for off in (1e3, 1e4, 1e5, 1e6):
        o = rng.uniform(-1.2, 1.2, size=(40, 3))
        ax = rng.integers(0, 3, 40)
        o[np.arange(40), ax] += off * rng.choice([-1, 1], 40)
        add(_sized_boxes(o, (7 * H, 7 * H, H)), "far")
    boxes = np.concatenate(out)
    assert (boxes[:, 0::2] <= boxes[:, 1::2]).all()
    return shape, tree, boxes, np.array(kinds), near


_CACHE = {}


def _case(oracle, name):
    """Boxes, sample points and the oracle's values for a tree, computed once and shared."""
    if name not in _CACHE:
        shape, tree, boxes, kinds, near = _make_boxes(oracle, name)
        pts = _box_points(boxes, 7)
        f = oracle.eval_implicit(tree, pts.reshape(-1, 3)).reshape(len(boxes), 64)
        f.setflags(write=False)
        _CACHE[name] = (shape, tree, boxes, kinds, near, pts, f)
    return _CACHE[name]


def _check_p1_p2(impli, shape, boxes, pts, f, iv, modes, what):
    nan = np.isnan(f)
    lo, hi = iv[:, :1], iv[:, 1:]
    assert not np.isnan(iv).any(), what
    ok = nan | ((lo <= f) & (f <= hi))
    bad = np.argwhere(~ok)
    assert bad.size == 0, (what, "P1", len(bad), [(int(b), int(k), float(f[b, k]), iv[b].tolist(), boxes[b].tolist()) for b, k in bad[:5]])
    fp = impli.debug_eval_modes(shape, pts.reshape(-1, 3), np.repeat(modes, 64)).reshape(f.shape)
    same = (fp.view(np.uint32) == f.view(np.uint32)) | (np.isnan(fp) & nan)
    bad = np.argwhere(~same)
    assert bad.size == 0, (what, "P2", len(bad), [(int(b), int(k), float(f[b, k]), float(fp[b, k]), hex(int(modes[b])), boxes[b].tolist()) for b, k in bad[:5]])


# ---- P1 + P2 (+ the NaN cap) ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TREES))
def test_bounds_contain_and_decisions_hold(impli, oracle, name):
    shape, tree, boxes, kinds, near, pts, f = _case(oracle, name)
    assert 1500 <= len(boxes) <= 4096
    assert np.isnan(f).mean() <= 1e-3, np.isnan(f).mean()     # the oracle alone stays within the cap
    iv, modes = impli.debug_intervals(shape, boxes, variant=0)
    _check_p1_p2(impli, shape, boxes, pts, f, iv, modes, name)
    # bounds that say something: a point box of a finite value is never the whole line
    pt = kinds == "point"
    fin = np.isfinite(f[pt]).all(1)
    assert np.isfinite(iv[pt][fin]).all(), name


# ---- P3 nesting -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TREES))
def test_nested_chain_inherits_modes(impli, oracle, name):
    """From the whole [-1.2, 1.2]^3 down five octant levels towards near-surface points: each level's
    modes_in is its parent's modes_out."""
    shape, tree, _, _, near, _, _ = _case(oracle, name)
    targets = near[:24].astype(np.float64)
    lo = np.full_like(targets, -1.2)
    hi = np.full_like(targets, 1.2)
    modes_in = None
    pruned = 0
    for level in range(6):
        boxes = np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1], lo[:, 2], hi[:, 2]], 1).astype(np.float32)
        pts = _box_points(boxes, 100 + level)
        f = oracle.eval_implicit(tree, pts.reshape(-1, 3)).reshape(len(boxes), 64)
        iv, modes = impli.debug_intervals(shape, boxes, variant=0, modes_in=modes_in)
        if modes_in is not None:   # decisions only accumulate: a pruned operand stays pruned
            for k in range(32):
                was = (modes_in >> np.uint64(2 * k)) & np.uint64(3)
                now = (modes >> np.uint64(2 * k)) & np.uint64(3)
                assert ((was == 0) | (was == now)).all(), (name, level, k)
        _check_p1_p2(impli, shape, boxes, pts, f, iv, modes, (name, "level", level))
        pruned = int((modes != 0).sum())
        modes_in = modes
        b32 = boxes.astype(np.float64)
        mid = (b32[:, 0::2] + b32[:, 1::2]) / 2
        up = targets >= mid
        lo = np.where(up, mid, b32[:, 0::2])
        hi = np.where(up, b32[:, 1::2], mid)
    if name in ("union_sphere_cube", "config3_tree"):
        assert pruned > 0, name    # small boxes of a CSG tree prune something


# ---- P4 variants ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CSG_TREES + ["rot_" + k for k in matrices.LEAF_TYPES])
def test_jit_variants_match_interpreter(impli, oracle, name):
    """tree_iv of the shape module and of the baked module against eval_iv.  Baked modules for the CSG
    trees only (hipRTC costs seconds per module); the rotated leaves run the shape module."""
    shape, tree, boxes, kinds, near, pts, f = _case(oracle, name)
    iv0, m0 = impli.debug_intervals(shape, boxes, variant=0)
    for variant in ((1, 2) if name in CSG_TREES else (1,)):
        iv, m = impli.debug_intervals(shape, boxes, variant=variant)
        assert np.array_equal(m, m0), (name, variant, np.flatnonzero(m != m0)[:10])
        bad = np.flatnonzero(~(iv == iv0).all(1))
        assert bad.size == 0, (name, variant, bad[:10], iv[bad[:3]], iv0[bad[:3]])


# ---- P5 point boxes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [k for k in MIRRORING if k not in P5_EXCEPTIONS])
def test_point_box_is_value_widened_by_settle(impli, oracle, kind):
    """lo == hi boxes under the identity: every interval operation is the point operation on a
    degenerate interval, so the bound is [f, f] widened by settle's s = |f| 2^-16 + 1e-30.
    hi - lo <= 2 s plus one float ulp at the magnitude of the endpoints: lo and hi are each the
    float rounding of f -+ s (half an ulp of the endpoint each), which is the only slack settle's
    own arithmetic adds."""
    shape, tree, boxes, kinds, near, pts, f = _case(oracle, "eye_" + kind)
    sel = kinds == "point"
    iv, _ = impli.debug_intervals(shape, boxes[sel], variant=0)
    fv = f[sel][:, 0].astype(np.float64)                       # every sample of a point box is the point
    assert (f[sel] == f[sel][:, :1]).all() or np.isnan(f[sel]).any()
    fin = np.isfinite(fv)
    assert fin.sum() >= 150
    lo, hi = iv[fin, 0].astype(np.float64), iv[fin, 1].astype(np.float64)
    fv = fv[fin]
    assert ((lo <= fv) & (fv <= hi)).all()
    ulp = np.spacing(np.maximum(np.abs(iv[fin, 0]), np.abs(iv[fin, 1])).astype(np.float32)).astype(np.float64)
    bound = 2 * (np.abs(fv) * 2.0 ** -16 + 1e-30) + ulp
    bad = np.flatnonzero(~(hi - lo <= bound))
    assert bad.size == 0, (kind, len(bad), [(fv[b], lo[b], hi[b], bound[b]) for b in bad[:5]])


# ---- P6 pruning power -------------------------------------------------------------------------------
def true_mixed_interior(field):
    """Bricks (8 x 8 x 2 stored samples) without a sealed sample (the first and the last stored index
    of every axis: the slab stores the samples 1 .. res - 2) whose samples truly hold both signs
    (MC's test: f < 0)."""
    L, ny, nx = field.shape
    neg = field < 0
    count = 0
    for bz in range((L + 1) // 2):
        for by in range((ny + 7) // 8):
            for bx in range((nx + 7) // 8):
                z0, z1 = 2 * bz, min(2 * bz + 2, L)
                y0, y1 = 8 * by, min(8 * by + 8, ny)
                x0, x1 = 8 * bx, min(8 * bx + 8, nx)
                if z0 < 1 or y0 < 1 or x0 < 1 or z1 > L - 1 or y1 > ny - 1 or x1 > nx - 1:
                    continue
                s = neg[z0:z1, y0:y1, x0:x1]
                count += bool(s.any() and not s.all())
    return count


def pruning_counts(impli, shape, R=32):
    """(true mixed interior bricks from the level-0 field, bricks the interval pass classes mixed)."""
    from implisolid_amd import scenes
    mc = scenes.mc_settings(R, 1.0)
    out = []
    try:
        for level in (0, 2):
            impli.set_pruning(level)
            s = impli.Slab(shape, mc)
            try:
                s.eval()
                out.append(s.read_field() if level == 0 else s.brick_stats())
            finally:
                s.close()
    finally:
        impli.set_pruning(2)
    return true_mixed_interior(out[0]), out[1][1], out[1][0]


@pytest.mark.parametrize("name", sorted(OBJECTS))
def test_pruning_power_not_worse_than_recorded(impli, name):
    """Deterministic integers, so no margin: fewer mixed bricks than recorded is allowed, more
    fails; fewer than the truly mixed ones would be unsound."""
    recorded = json.load(open(GOLDEN))["mixed_bricks_r32"][name]
    true_mixed, mixed, bricks = pruning_counts(impli, OBJECTS[name])
    assert 0 < true_mixed <= mixed <= recorded < bricks, (name, true_mixed, mixed, recorded, bricks)
