"""The claims of the brick eval kernel, one direction per lane (eval_bricks.hpp claim_neighbours): lanes
0-5 of a mixed brick's wave load their neighbours' fill bytes, test their faces, claim with one atomic
instruction and load their candidates' modes.  Small grids chosen for where a per-lane claim can go
wrong; in each the level-2 mesh must be the level-0 mesh bit for bit, and the interpreter and the JIT
module must agree on field, sign words, brick statistics and fill bytes (claimed flags included).

The claimed set is also restated on the host from the level-0 signs and the fill bytes' classes and
candidate flags: a candidate is claimed exactly when a mixed face neighbour holds, on the shared face,
a sample of the other sign.  The claimed flags must be that set, every claimed brick's values must be
the dense field's, and each direction a case is meant to cover must hold at least one claim (the
counts go into the assert message).
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BX, BY, BZ = 8, 8, 2
CAND, CLAIMED = 0x08, 0x80
DIRS = ("-x", "+x", "-y", "+y", "-z", "+z")
EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def _plane(normal, point):
    return {"type": "half_plane", "matrix": list(EYE), "plane_vector": list(normal), "plane_point": list(point)}


def _cut_sphere():
    # radius 1.3 in the +-1 box: the surface meets all six box faces; cut through the centre
    from implisolid_amd import scenes
    return {"type": "Intersection", "matrix": list(EYE), "children": [
        {"type": "iellipsoid", "matrix": scenes.st(2.6, 0, 0, 0)}, _plane([1, 2, 3], [0, 0, 0])]}


def _slab(deg, z0=0.0):
    # 0.12 thick (2.4 sample spacings at R = 40), `deg` degrees off the xy plane
    a = math.radians(deg)
    n = [math.sin(a), 0.0, math.cos(a)]
    return {"type": "Intersection", "matrix": list(EYE), "children": [
        _plane(n, [0, 0, z0 - 0.06]), _plane([-n[0], 0.0, -n[2]], [0, 0, z0 + 0.06])]}


def _tilted_slab():
    # two thin slabs tilted 5 degrees either way, at different heights: the mixed bands step in z both
    # ways along x, with sign-definite bricks above and below it
    return {"type": "Union", "matrix": list(EYE), "children": [_slab(5.0, 0.05), _slab(-5.0, -0.3)]}


def _x_slab():
    # 0.36 thick in x (7.2 sample spacings at R = 40: a mixed band one brick thick in x), 3 degrees off
    # the yz plane, so that along z it drifts 2 spacings through brick column 2 (samples 16-23, x from
    # -0.25 to 0.10): where it fills the column's first and last sample and no more, the brick's -x and
    # +x neighbours are both sign-definite candidates and both wanted
    a = math.radians(3.0)
    n = [math.cos(a), 0.0, math.sin(a)]
    return {"type": "Intersection", "matrix": list(EYE), "children": [
        _plane(n, [-0.075 - 0.18, 0, 0]), _plane([-n[0], 0.0, -n[2]], [-0.075 + 0.18, 0, 0])]}


def _staircase():
    from implisolid_amd import scenes
    return {"type": "Union", "matrix": list(EYE), "children": [
        scenes.extrusion(4, 0.45, (-0.55 + 0.22 * k, 0.5 - 0.19 * k, -0.5 + 0.21 * k)) for k in range(6)]}


def _union():
    from implisolid_amd import scenes
    return scenes.union_sphere_cube()


# name: (shape, R, directions that must each hold a claim)
CASES = {
    "cut_sphere_R32": (_cut_sphere, 32, DIRS),
    "union_R37": (_union, 37, DIRS),
    # (its interval pass lists the bricks at the band's steps in x: the x claims are the sphere's and the union's)
    "tilted_slab_R40": (_tilted_slab, 40, ("-z", "+z")),
    # one wave's -x and +x claims in one 32-bit fill word (two lanes' atomics on one address)
    "x_slab_R40": (_x_slab, 40, ("-x", "+x")),
    "staircase_R40": (_staircase, 40, ()),   # what it must hold: a candidate wanted by two mixed bricks
}


@pytest.fixture
def knobs(impli):
    yield impli
    impli.set_jit(2)
    impli.set_jit_bake(2)
    impli.set_pruning(2)


def _run(I, shape, mc, level, jit, rank=0, world=1):
    """One slab at the given pruning level through the interpreter (jit = 0) or the shape module."""
    I.set_pruning(level)
    I.set_jit(jit)
    I.set_jit_bake(0)
    s = I.Slab(shape, mc, rank, world)
    try:
        nv, nf = s.run()
        assert s.used_jit() == bool(jit and level)
        v, f = s.download(nv, nf)
        return {"v": v, "f": f, "field": s.read_field(), "signs": s.read_signs(), "stats": s.brick_stats(),
                "fill": s.read_fill()}
    finally:
        s.close()


def _expected_claims(fill, signs):
    """The bricks the claim rule claims, per direction the (mixed brick, candidate) pairs that want a
    claim, and the number of mixed bricks b that want both b - 1 and b + 1 with the two fill bytes in
    one 32-bit word: restated from the level-0 signs (layers, n, n) and the fill bytes (nbz, nby, nbx)."""
    nbz, nby, nbx = fill.shape
    layers, n, _ = signs.shape
    neg = signs.astype(bool)
    want = np.zeros(fill.shape, np.int32)      # how many mixed neighbours want each candidate
    per_dir = [0] * 6
    one_word = 0
    for bz in range(nbz):
        for by in range(nby):
            for bx in range(nbx):
                if fill[bz, by, bx] & 3:       # only mixed (listed, checked) bricks claim
                    continue
                blk = neg[bz * BZ:(bz + 1) * BZ, by * BY:(by + 1) * BY, bx * BX:(bx + 1) * BX]
                full = blk.shape == (BZ, BY, BX)
                wanted = 0
                for d in range(6):
                    ax, up = d >> 1, d & 1
                    c = (bx, by, bz)[ax] + (1 if up else -1)
                    if c < 0 or c >= (nbx, nby, nbz)[ax]:
                        continue
                    a = (bz + (ax == 2) * (2 * up - 1), by + (ax == 1) * (2 * up - 1), bx + (ax == 0) * (2 * up - 1))
                    if not fill[a] & CAND:
                        continue
                    # a brick with a neighbour above it on an axis is whole along that axis
                    assert not up or blk.shape[2 - ax] == (BX, BY, BZ)[ax], (full, d)
                    face = blk.take(-1 if up else 0, axis=2 - ax)
                    cand_neg = (fill[a] & 3) == 2
                    if (face != cand_neg).any():
                        want[a] += 1
                        per_dir[d] += 1
                        wanted |= 1 << d
                b = bx + nbx * (by + nby * bz)
                one_word += (wanted & 3) == 3 and (b - 1) >> 2 == (b + 1) >> 2
    return want, per_dir, one_word


def _brick_values(field, b):
    bz, by, bx = b
    return field[bz * BZ:(bz + 1) * BZ, by * BY:(by + 1) * BY, bx * BX:(bx + 1) * BX]


def _check_case(I, shape, mc, need, rank=0, world=1, shared_candidate=False, one_word=False, any_claim=True):
    dense = _run(I, shape, mc, 0, 0, rank, world)
    assert len(dense["f"]) > 0
    runs = {jit: _run(I, shape, mc, 2, jit, rank, world) for jit in (0, 1)}
    a, b = runs[0], runs[1]
    # interpreter against the JIT module
    assert np.array_equal(a["field"].view(np.uint32), b["field"].view(np.uint32))
    assert np.array_equal(a["signs"], b["signs"])
    assert a["stats"] == b["stats"]
    assert np.array_equal(a["fill"], b["fill"])
    for r in (a, b):
        assert np.array_equal(r["signs"], dense["signs"])
        assert r["f"].shape == dense["f"].shape and np.array_equal(r["f"], dense["f"])
        assert np.array_equal(r["v"].view(np.uint32), dense["v"].view(np.uint32))
    fill = b["fill"]
    want, per_dir, same_word = _expected_claims(fill, dense["signs"])
    counts = dict(zip(DIRS, per_dir))
    claimed = (fill & CLAIMED) != 0
    assert np.array_equal(claimed, want > 0), "claimed %d bricks, the rule claims %d (%s)" % (
        claimed.sum(), (want > 0).sum(), counts)
    assert sum(per_dir) > 0 or not any_claim, "no claim at all: %s" % counts
    for d in need:
        assert counts[d] > 0, "no claim in direction %s: %s" % (d, counts)
    if one_word:
        assert same_word > 0, "%d bricks claim -x and +x in one fill word: %s" % (same_word, counts)
    if shared_candidate:
        assert (want > 1).any(), "no candidate is wanted by two mixed bricks: %s" % counts
    # claimed and listed bricks hold the dense field's values
    for r in (a, b):
        for bk in zip(*np.nonzero(claimed | (((fill >> 4) & 3) == 0))):
            assert np.array_equal(_brick_values(r["field"], bk).view(np.uint32),
                                  _brick_values(dense["field"], bk).view(np.uint32)), bk
    # brick_stats' sign-filled count leaves the claimed bricks out
    assert b["stats"][2] == int(((((fill >> 4) & 3) != 0) & ~claimed).sum())
    return counts


@pytest.mark.parametrize("name", sorted(CASES))
def test_claims_single_slab(knobs, name):
    from implisolid_amd import scenes
    make, R, need = CASES[name]
    _check_case(knobs, make(), scenes.mc_settings(R, 1.0), need, shared_candidate=name.startswith("staircase"),
                one_word=name.startswith("x_slab"))


# (scene, rank, directions that must each hold a claim, whether the slab must hold a claim at all)
THREE_SLABS = [
    # the staircase: its lowest slab holds one cube's underside and no candidate beside a crossing
    ("staircase", 0, (), False), ("staircase", 1, (), True), ("staircase", 2, (), True),
    # the cut sphere: the slabs with fz0 != 0 claim across z both ways
    ("cut_sphere", 0, ("-z",), True), ("cut_sphere", 1, ("-z", "+z"), True), ("cut_sphere", 2, ("-z", "+z"), True),
    # the x slab's middle slab: one wave's -x and +x claims in one fill word, at a brick z offset
    ("x_slab", 1, ("-x", "+x"), True),
]


@pytest.mark.parametrize("scene,rank,need,any_claim", THREE_SLABS)
def test_claims_in_three_slabs(knobs, scene, rank, need, any_claim):
    """Non-zero fz0, the halo layer and brick z offsets: three Z-slabs at R = 40."""
    from implisolid_amd import scenes
    make = {"staircase": _staircase, "cut_sphere": _cut_sphere, "x_slab": _x_slab}[scene]
    _check_case(knobs, make(), scenes.mc_settings(40, 1.0), need, rank=rank, world=3, any_claim=any_claim,
                one_word=scene == "x_slab")


def test_claims_merged_object_stream(knobs):
    """The deferred path (eval_listed_deferred: claims appended for a second launch): four small
    objects at R = 32 in merged launches give the per-object builds' meshes.  Each object has claims:
    its own level-2 build through the interpreter sets claimed flags."""
    from implisolid_amd import scenes
    I = knobs
    mc = scenes.mc_settings(32, 1.0)
    shapes = [_cut_sphere(), _union(), _staircase(), scenes.random_tree(7301, 3)]
    I.set_pruning(2)
    with I.Batch(shapes, mc, n_streams=0) as bt:
        assert bt.merged
        bt.run()
        got = [bt.download(i) for i in range(len(shapes))]
    for k, (shape, (v, f)) in enumerate(zip(shapes, got)):
        ref = _run(I, shape, mc, 0, 0)
        assert len(ref["f"]) > 0
        assert f.shape == ref["f"].shape and np.array_equal(f, ref["f"])
        assert np.array_equal(v.view(np.uint32), ref["v"].view(np.uint32))
        n_claimed = int(((_run(I, shape, mc, 2, 0)["fill"] & CLAIMED) != 0).sum())
        assert n_claimed > 0, "object %d claims %d candidates" % (k, n_claimed)
