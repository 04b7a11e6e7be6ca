"""What tests/test_gpu_nonfinite.py relies on, asserted on the oracle's field alone.  No GPU.

The inputs are tests/nonfinite_inputs.py's: trees with one leaf whose arithmetic overflows at finite points.
An edit that spoils one (a scale at which the field is finite again, a plane that misses the NaN region)
fails here.  Every count is a condition on the inputs, not on the code under test.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonfinite_inputs as nf   # noqa: E402
import np_islands   # noqa: E402
import np_mass   # noqa: E402
import np_raster   # noqa: E402
import np_raycast   # noqa: E402
import np_rayspans   # noqa: E402
import np_slice   # noqa: E402
import ray_edge_inputs as edges   # noqa: E402

ENOUGH = 100


def _tables(oracle, name):
    """every field table of the case: (what, F)"""
    out = [(("raster",) + g, nf.raster_field(oracle, name, *g)) for g in nf.GRIDS]
    out += [(("slice", R), nf.slice_field(oracle, name, R)) for R in nf.SLICE_R]
    out += [(("mass", d), nf.mass_field(oracle, name, d)) for d in nf.DEPTHS]
    out += [(("rays", 130), nf.ray_field(oracle, nf.ray_case(name, 130)))]
    return out


@pytest.mark.parametrize("name", nf.NAMES)
def test_every_table_holds_the_classes_the_case_claims(oracle, name):
    for what, F in _tables(oracle, name):
        c = nf.classes(F)
        counts = {k: int(v.sum()) for k, v in c.items()}
        print(name, what, counts)
        assert sum(counts.values()) == F.size
        for k in nf.CLAIMS[name]:
            assert counts[k] >= ENOUGH, (name, what, k, counts)
    assert nf.CLAIMS[name] & {"nan", "pinf", "ninf"}, "every case holds a class that is not finite"


def test_the_mixed_cases_and_the_claimed_infinities():
    assert {"inter", "cone", "shear", "deep"} <= set(nf.MIXED)
    assert "pinf" in nf.CLAIMS["union_sl"] and "ninf" in nf.CLAIMS["diff"] and "nan" in nf.CLAIMS["diff"]


def test_the_order_pair_differs_where_the_leaf_is_nan(oracle):
    a, b = nf.ORDER_PAIR
    for (what, Fa), (_, Fb) in zip(_tables(oracle, a), _tables(oracle, b)):
        differ = Fa.view(np.uint32) != Fb.view(np.uint32)
        dropped = np.isnan(Fa) & np.isfinite(Fb)
        print(what, "differ", int(differ.sum()), "NaN against finite", int(dropped.sum()))
        assert dropped.sum() >= ENOUGH and np.array_equal(differ, np.isnan(Fa)), "they differ exactly where Union(sphere, leaf) is NaN"
        with np.errstate(invalid="ignore"):
            assert (Fb[dropped] < 0).sum() >= ENOUGH, "and there a solid sample of one is an empty one of the other"


def _edge_pairs(F):
    """(a, b) float32 (m,) each: the two samples of every cell edge of the slice fields F (L, R + 1, R + 1)"""
    return (np.concatenate([F[:, :, :-1].reshape(-1), F[:, :-1, :].reshape(-1)]),
            np.concatenate([F[:, :, 1:].reshape(-1), F[:, 1:, :].reshape(-1)]))


def _joins(F, ka, kb):
    a, b = _edge_pairs(F)
    ca, cb = nf.classes(a), nf.classes(b)
    return int(((ca[ka] & cb[kb]) | (ca[kb] & cb[ka])).sum())


@pytest.mark.parametrize("R", nf.SLICE_R)
def test_slice_edges_join_finite_and_non_finite_samples(oracle, R):
    for name in nf.MIXED:
        assert _joins(nf.slice_field(oracle, name, R), "neg", "nan") >= 1, (name, "an edge from finite negative to NaN: mu is NaN")
    assert _joins(nf.slice_field(oracle, "union_ls", R), "neg", "pinf") >= 1, "an edge from finite negative to +Inf: mu is +-0"
    for name in ("diff", "shear"):   # the cases that offer it
        F = nf.slice_field(oracle, name, R)
        assert _joins(F, "ninf", "nan") + _joins(F, "ninf", "pos") + _joins(F, "ninf", "pinf") >= 1, (name, "an edge from -Inf to a solid sample")
    # what the header's formula gives on such edges, under IEEE arithmetic
    with np.errstate(all="ignore"):
        f = np.float32
        mu = lambda a, b: (f(0) - f(a)) / (f(b) - f(a))   # noqa: E731
        assert np.isnan(mu(-1, np.nan)) and np.isnan(mu(-np.inf, 1)) and np.isnan(mu(-np.inf, np.inf)) and mu(-1, np.inf) == 0


@pytest.mark.parametrize("name", nf.MIXED)
def test_a_tile_and_a_leaf_box_hold_nan_and_finite_negative_samples(oracle, name):
    def both(F, items):
        c = nf.classes(F)
        return sum(bool(c["nan"][it[0], it[1], it[2]].any() and c["neg"][it[0], it[1], it[2]].any()) for it in items)
    for g in nf.GRIDS:
        assert both(nf.raster_field(oracle, name, *g), nf.raster_tiles(*g)) >= 1, (name, g)
    for R in nf.SLICE_R:
        assert both(nf.slice_field(oracle, name, R), nf.slice_tiles(R)) >= 1, (name, R)
    if name == "inter":
        return   # its NaN region starts at x = 0.75, an edge of every level of the box +-1: no mass box holds both
    for d in nf.DEPTHS:
        assert both(nf.mass_field(oracle, name, d), nf.mass_boxes(d)) >= 1, (name, d)


def test_the_cone_s_border_crosses_tile_interiors(oracle):
    """NaN and finite samples of both signs strictly inside one raster tile's rows and columns"""
    W, H, s = nf.GRIDS[0]
    F = nf.raster_field(oracle, "cone", W, H, s)
    c = nf.classes(F)
    hit = 0
    for l, ys, xs, _ in nf.raster_tiles(W, H, s):
        inner = (l, slice(ys.start + 1, ys.stop - 1), slice(xs.start + 1, xs.stop - 1))
        hit += bool(c["nan"][inner].any() and c["neg"][inner].any() and c["pos"][inner].any())
    assert hit >= 1


@pytest.mark.parametrize("name", nf.NAMES)
def test_local_coordinates_stay_far_below_overflow(oracle, name):
    """program.hpp's documented limit is a transformed coordinate that is itself infinite; here every leaf's
    coordinates stay below 2^100 and the overflow happens inside the primitive"""
    pts = [nf.raster_table(*nf.GRIDS[0])[2], nf.slice_table(nf.SLICE_R[0])[2], np_mass.points(np_mass.mids(nf.BOX, nf.DEPTHS[-1]))]
    c = nf.ray_case(name, 130)
    pts.append(np_raycast.points(c.o, c.d, np.broadcast_to(c.ts[None, :], (len(c), len(c.ts)))).reshape(-1, 3))
    for P in pts:
        for kind, Q in nf.leaves_local(nf.TREES[name], P):
            assert np.isfinite(Q).all() and np.abs(Q).max() < nf.LIMIT, (name, kind, np.abs(Q).max())
    big = max(np.abs(Q).max() for _, Q in nf.leaves_local(nf.TREES[name], pts[0]))
    assert big >= 2.0 ** 63, "and one leaf's are large enough for its arithmetic to overflow"


def test_one_leaf_is_sheared_and_one_tree_is_deep():
    m = nf.HEART_SHEARED["matrix"]
    assert m[1] != 0 and m[0] == m[5] == m[10] == nf.SCALE, "an off-diagonal entry of the scale's magnitude: XF_GENERIC"

    def depth(n):   # operands on the stack: the second child is evaluated over the first one's value
        return 1 if "children" not in n else max(depth(n["children"][0]), 1 + depth(n["children"][1]))
    assert depth(nf.TREES["deep"]) > 12 and depth(nf.TREES["shear"]) <= 12


@pytest.mark.parametrize("name", nf.NAMES)
def test_the_restatements_accept_the_fields(oracle, name):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        W, H, s = nf.GRIDS[0]
        cov, sums = np_raster.coverage(nf.raster_field(oracle, name, W, H, s), s)
        assert sums.sum() > 0
        for threshold in (1, s * s):
            offs, comps, lab = np_islands.islands(cov, threshold, 8)
            assert offs[-1] == len(comps)
        m, layers = np_mass.moments(nf.mass_field(oracle, name, nf.DEPTHS[0]))
        assert m[0] == layers.sum() > 0
        R = nf.SLICE_R[1]
        xs, ys, _ = nf.slice_table(R)
        seg, keys, so = np_slice.march(nf.slice_field(oracle, name, R), xs, ys)
        assert so[-1] == len(seg) > 0
        for l in range(len(nf.Z)):
            assert np_slice.loops(keys[so[l]:so[l + 1]]) is not None, "NaN corners still chain: the cases come from the solid bits"
        if name in nf.MIXED:
            assert np.isnan(seg).any() and np.isfinite(seg).any(), "vertices of both kinds"
        c = nf.ray_case(name, 130)
        F = nf.ray_field(oracle, c)
        fn = edges._field_fn(None, oracle, "oracle", c.shape)
        hit, t, f = np_raycast.cast(fn, c.o, c.d, c.ts, 24, F=F)
        o2, k, st, sf = np_rayspans.spans(fn, c.o, c.d, c.ts, 24, F=F)
        assert (hit >= 0).any() and o2[-1] == len(k)


def _ray_refs(oracle, name, N=130, B=24):
    c = nf.ray_case(name, N)
    F = nf.ray_field(oracle, c)
    fn = edges._field_fn(None, oracle, "oracle", c.shape)
    return c, F, np_raycast.cast(fn, c.o, c.d, c.ts, B, F=F), np_rayspans.spans(fn, c.o, c.d, c.ts, B, F=F)


@pytest.mark.parametrize("name", ["inter", "shear", "deep", "cone"])
def test_the_rays_hold_the_cases_the_gpu_tests_name(oracle, name):
    c, F, (hit, t, f), (offs, k, st, sf) = _ray_refs(oracle, name)
    rows = np.arange(len(c))
    # a bisection whose solid end is a NaN sample: a bracket from a sample < 0 to a NaN one, and f stays NaN
    bracket = (hit >= 1) & np.isnan(F[rows, np.maximum(hit, 0)])
    print(name, "rays", len(c), "hits", int((hit >= 0).sum()), "brackets onto NaN", int(bracket.sum()))
    assert bracket.sum() >= 3 and np.isnan(f[bracket]).all()
    assert ((hit >= 1) & np.isfinite(f)).sum() >= 3 and (hit < 0).sum() >= 1 and (hit == 0).sum() >= 1
    # a span that opens on a NaN sample and closes on a finite one
    ray = np.repeat(rows, np.diff(offs))
    first, last = F[ray, k[:, 0]], F[ray, k[:, 1] - 1]
    opens_nan = np.isnan(first) & np.isfinite(last)
    print(name, "spans", len(k), "open on NaN and close on finite", int(opens_nan.sum()))
    if name != "inter":    # the iheart's NaN region under scale and translate does not touch the sphere
        assert opens_nan.sum() >= 1
    assert (np.isnan(first) & (k[:, 0] >= 1)).sum() >= 3 and (np.isfinite(first) & np.isfinite(last)).sum() >= 3


@pytest.mark.parametrize("name", nf.LATE_NAMES)
def test_the_late_rays_enter_the_nan_region_in_the_second_batch(oracle, name):
    c = nf.late_case(name)
    F = nf.ray_field(oracle, c)
    with np.errstate(invalid="ignore"):
        solid = ~(F < 0)
    first_nan = np.where(np.isnan(F).any(1), np.isnan(F).argmax(1), -1)
    print(name, "first NaN sample per ray", first_nan.tolist())
    assert (first_nan > 4096).sum() >= 2 and c.N == 4200
    assert (solid.argmax(1)[first_nan > 4096] > 4096).any(), "a ray whose first solid sample is that NaN"
