"""Fields that are not finite at finite points (NaN, +Inf, -Inf), through every grid and ray query on the GPU.

The inputs are tests/nonfinite_inputs.py's: trees with one leaf under a matrix of scale 2^-64 .. 2^-66 whose
arithmetic overflows inside the primitive (tests/test_cpu_nonfinite.py asserts what they hold, on the
oracle's field alone).  The reference is always the query's numpy restatement fed with the oracle's field,
never a kernel's output.  Every comparison is an integer equality, same_bits (the bits, Inf included, and NaN
by position: a NaN's sign and payload are the producer's, and the oracle is x86 C), at pruning levels 0 and
2, and the two levels' results are compared with each other.

What this pins and the other suites do not: solidity is !(F < 0), so a NaN sample is solid (f >= 0 makes it
empty); the CSG selects keep a NaN in one operand position and drop it in the other, under the pruned
interpreters' modes words as well; the interval interpreter stays sound over boxes that hold NaN and Inf
samples (a non-finite primitive bound becomes the whole line before a CSG node sees it); the slicer's
vertices on edges whose mu is not finite are what the header's formula gives.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nonfinite_inputs as nf   # noqa: E402
import np_bounds   # noqa: E402
import np_islands   # noqa: E402
import np_mass   # noqa: E402
import np_raster   # noqa: E402
import np_raycast   # noqa: E402
import np_slice   # noqa: E402
import ray_edge_inputs as edges   # noqa: E402
import rayspan_inputs as spans_in   # noqa: E402
import test_gpu_raycast as tg   # noqa: E402  (its checks; its tests are not collected from here)
import test_gpu_rayspans as ts_   # noqa: E402
from np_normals import same_bits   # noqa: E402

pytestmark = pytest.mark.gpu

LEVELS = nf.LEVELS
BOXES_PER_CALL = 4096
_CACHE = {}


def _at(impli, level, fn, *a, **kw):
    impli.set_pruning(level)
    try:
        return fn(*a, **kw)
    finally:
        impli.set_pruning(2)


def _intervals(impli, name, boxes):
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    out = [impli.debug_intervals(nf.TREES[name], boxes[i:i + BOXES_PER_CALL]) for i in range(0, len(boxes), BOXES_PER_CALL)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def _box_sets(oracle, name):
    """[(kind, boxes (n, 6), [points (m, 3) per box], [oracle's F (m,) per box])]: the very boxes the queries
    bound, each with the query's own samples inside it"""
    def make():
        out = []
        W, H, s = nf.GRIDS[0]
        P = nf.raster_table(W, H, s)[2].reshape(len(nf.Z), H * s, W * s, 3)
        F = nf.raster_field(oracle, name, W, H, s)
        items = nf.raster_tiles(W, H, s)
        out.append(("raster", [it[3] for it in items], [P[it[0], it[1], it[2]].reshape(-1, 3) for it in items],
                    [F[it[0], it[1], it[2]].reshape(-1) for it in items]))
        R = nf.SLICE_R[1]
        P = nf.slice_table(R)[2].reshape(len(nf.Z), R + 1, R + 1, 3)
        F = nf.slice_field(oracle, name, R)
        items = nf.slice_tiles(R)
        out.append(("slice", [it[3] for it in items], [P[it[0], it[1], it[2]].reshape(-1, 3) for it in items],
                    [F[it[0], it[1], it[2]].reshape(-1) for it in items]))
        d = nf.DEPTHS[0]
        N = 1 << d
        P = np_mass.points(np_mass.mids(nf.BOX, d)).reshape(N, N, N, 3)
        F = nf.mass_field(oracle, name, d)
        items = nf.mass_boxes(d)
        out.append(("mass", [it[3] for it in items], [P[it[0], it[1], it[2]].reshape(-1, 3) for it in items],
                    [F[it[0], it[1], it[2]].reshape(-1) for it in items]))
        c = nf.ray_case(name, 130)
        F = nf.ray_field(oracle, c)
        P = np_raycast.points(c.o, c.d, np.broadcast_to(c.ts[None, :], (len(c), len(c.ts))))
        B = edges.segment_boxes(c)
        boxes, pts, fs = [], [], []
        for r in range(len(c)):
            for j in range(edges.nseg(c.N)):
                k0, k1 = 64 * j, min(64 * j + 64, c.N) + 1   # the samples between the box's end samples, both included
                boxes.append(B[r, j])
                pts.append(P[r, k0:k1])
                fs.append(F[r, k0:k1])
        out.append(("rays", boxes, pts, fs))
        return [(k, np.array(b, np.float32).reshape(-1, 6), p, f) for k, b, p, f in out]
    return nf._cached(("box_sets", name), make)


def _bounded(impli, oracle, name):
    """[(kind, boxes, pts, fs, iv, modes)], the interval interpreter run once per tree"""
    key = ("bounded", name)
    if key not in _CACHE:
        _CACHE[key] = [(k, b, p, f) + _intervals(impli, name, b) for k, b, p, f in _box_sets(oracle, name)]
    return _CACHE[key]


# ---- the field -------------------------------------------------------------------------------------------------------
def test_the_deep_tree_runs_the_16_slot_stacks(impli):
    assert impli.program_info(nf.TREES["deep"])[1] > 12 and impli.program_info(nf.TREES["shear"])[1] <= 12


@pytest.mark.parametrize("name", nf.NAMES)
def test_eval_equals_the_oracle(impli, oracle, name):
    tables = [(nf.raster_table(*nf.GRIDS[0])[2], nf.raster_field(oracle, name, *nf.GRIDS[0])),
              (nf.slice_table(nf.SLICE_R[1])[2], nf.slice_field(oracle, name, nf.SLICE_R[1])),
              (np_mass.points(np_mass.mids(nf.BOX, nf.DEPTHS[0])), nf.mass_field(oracle, name, nf.DEPTHS[0]))]
    c = nf.ray_case(name, 130)
    tables.append((np_raycast.points(c.o, c.d, np.broadcast_to(c.ts[None, :], (len(c), len(c.ts)))).reshape(-1, 3), nf.ray_field(oracle, c)))
    with impli.ImplicitService(nf.TREES[name]) as svc:
        for pts, F in tables:
            got = svc.eval(pts)
            F = F.reshape(-1)
            bad = np.flatnonzero(~((got.view(np.uint32) == F.view(np.uint32)) | (np.isnan(got) & np.isnan(F))))
            assert len(bad) == 0, (name, len(bad), pts[bad[:3]].tolist(), got[bad[:3]].tolist(), F[bad[:3]].tolist())
            assert np.array_equal(np.isnan(got), np.isnan(F)), "NaN exactly where the oracle's is NaN"


@pytest.mark.parametrize("name", nf.NAMES)
def test_the_pruned_interpreter_under_the_boxes_modes_equals_the_oracle(impli, oracle, name):
    decided = 0
    for kind, boxes, pts, fs, iv, modes in _bounded(impli, oracle, name):
        P, F = np.concatenate(pts), np.concatenate(fs)
        M = np.repeat(modes, [len(p) for p in pts])
        got = impli.debug_eval_modes(nf.TREES[name], P, M)
        bad = np.flatnonzero(~((got.view(np.uint32) == F.view(np.uint32)) | (np.isnan(got) & np.isnan(F))))
        print(name, kind, "boxes", len(boxes), "modes words not 0", int((modes != 0).sum()), "points", len(P))
        assert len(bad) == 0, (name, kind, len(bad), P[bad[:3]].tolist(), got[bad[:3]].tolist(), F[bad[:3]].tolist(), [hex(int(m)) for m in M[bad[:3]]])
        decided += int((modes != 0).sum())
    if name == "cone":   # the iheart is not finite anywhere in the box: its bound is the whole line and no node is decided
        assert decided > 0, "somewhere the bounds decide a CSG node"


# ---- the intervals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nf.NAMES)
def test_no_decisive_bound_contradicts_a_sample(impli, oracle, name):
    total = np.zeros(3, np.int64)
    for kind, boxes, pts, fs, iv, modes in _bounded(impli, oracle, name):
        with np.errstate(invalid="ignore"):
            outside, solid = iv[:, 1] < 0, iv[:, 0] >= 0
            any_solid = np.array([bool((~(f < 0)).any()) for f in fs])
            any_out = np.array([bool((f < 0).any()) for f in fs])
            holds_nonfinite = np.array([bool((~np.isfinite(f)).any()) for f in fs])
        assert not (outside & solid).any()
        bad = np.flatnonzero(outside & any_solid)
        assert len(bad) == 0, (name, kind, "proved outside, yet a sample is solid", boxes[bad[:3]].tolist(), iv[bad[:3]].tolist())
        bad = np.flatnonzero(solid & any_out)
        assert len(bad) == 0, (name, kind, "proved solid, yet a sample is < 0", boxes[bad[:3]].tolist(), iv[bad[:3]].tolist())
        counts = [int(outside.sum()), int(solid.sum()), int((~outside & ~solid).sum())]
        print(name, kind, "outside, solid, mixed", counts, "decisive over non-finite samples", int(((outside | solid) & holds_nonfinite).sum()))
        total += counts
    if name == "cone":   # the tree whose leaf is finite somewhere; an iheart tree's boxes are all mixed
        assert (total > 0).all(), (name, total.tolist(), "both decisive classes and the mixed class occur")
    assert total[2] > 0


# ---- mass --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", nf.DEPTHS)
@pytest.mark.parametrize("name", nf.NAMES)
def test_mass_moments_equal_the_restatement(impli, oracle, name, depth):
    F = nf.mass_field(oracle, name, depth)
    want = np_mass.moments(F)
    got = {}
    for level in LEVELS:
        mom, layers, stats = _at(impli, level, impli.mass_moments, nf.TREES[name], nf.BOX, depth, return_stats=True)
        print(name, depth, level, "cells", int(mom[0]), "of which NaN", int(np.isnan(F).sum()), "stats", stats)
        assert [int(v) for v in mom] == want[0], ([int(v) for v in mom], want[0])
        assert np.array_equal(layers, want[1])
        got[level] = (mom, layers)
    assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1])
    if "nan" in nf.CLAIMS[name]:
        with np.errstate(invalid="ignore"):
            assert want[0][0] > int((F >= 0).sum()), "the NaN cells are counted"


# ---- raster and islands ---------------------------------------------------------------------------------------------------
def _cov(oracle, name, W, H, s):
    return nf._cached(("cov", name, W, H, s), lambda: np_raster.coverage(nf.raster_field(oracle, name, W, H, s), s))


@pytest.mark.parametrize("W, H, s", nf.GRIDS)
@pytest.mark.parametrize("name", nf.NAMES)
def test_raster_images_equal_the_restatement(impli, oracle, name, W, H, s):
    want = _cov(oracle, name, W, H, s)
    got = {}
    for level in LEVELS:
        got[level] = _at(impli, level, impli.raster_layers, nf.TREES[name], nf.RECT, W, H, nf.Z, s, return_stats=True)
        print(name, (W, H, s), level, "sums", got[level][1].tolist(), "stats", got[level][2])
        import test_gpu_raster as gr
        gr._check_bits(got[level], want, W, H, s)
    assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1])
    assert 0 < want[1].sum() < len(nf.Z) * W * H * s * s


@pytest.mark.parametrize("W, H, s", nf.GRIDS)
@pytest.mark.parametrize("name", nf.NAMES)
def test_islands_equal_the_restatement(impli, oracle, name, W, H, s):
    import test_gpu_islands as gi
    cov = _cov(oracle, name, W, H, s)[0]
    for threshold in (1, s * s):
        for connectivity in (4, 8):
            want = nf._cached(("islands", name, W, H, s, threshold, connectivity), lambda: np_islands.islands(cov, threshold, connectivity))
            got = {}
            for level in LEVELS:
                got[level] = _at(impli, level, impli.layer_islands, nf.TREES[name], nf.RECT, W, H, nf.Z, s, threshold, connectivity,
                                 want_labels=True, return_stats=True)
                gi._check(impli, got[level], want)
            print(name, (W, H, s), threshold, connectivity, "per layer", np.diff(got[2][0]).tolist())
            assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1]) and np.array_equal(got[0][2], got[2][2])
    if name in nf.MIXED:
        rows = want[1]
        assert ((rows[:, 7] > 0) & (rows[:, 2] > 0)).any() and ((rows[:, 7] > 0) & (rows[:, 2] < rows[:, 1])).any(), \
            "components that rest on the layer below, and some only in part"


def test_islands_in_chunks_give_the_same_records(impli, oracle, monkeypatch):
    import test_gpu_islands as gi
    W, H, s = nf.GRIDS[0]
    want = np_islands.islands(_cov(oracle, "shear", W, H, s)[0], 1, 8)
    monkeypatch.setenv("IMPLISOLID_ISLANDS_CHUNK", "18")   # two layers of nine raster tiles
    got = impli.layer_islands(nf.TREES["shear"], nf.RECT, W, H, nf.Z, s, 1, 8, want_labels=True, return_stats=True)
    monkeypatch.delenv("IMPLISOLID_ISLANDS_CHUNK")
    assert got[3][4] == 4
    gi._check(impli, got, want)


# ---- slices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", nf.SLICE_R)
@pytest.mark.parametrize("name", nf.NAMES)
def test_slices_equal_the_restatement(impli, oracle, name, R):
    xs, ys, _ = nf.slice_table(R)
    seg_r, keys_r, offs_r = nf._cached(("march", name, R), lambda: np_slice.march(nf.slice_field(oracle, name, R), xs, ys))
    got = {}
    for level in LEVELS:
        seg, keys, offs, stats = _at(impli, level, impli.slice_layers, nf.TREES[name], nf.RECT, R, nf.Z, return_stats=True)
        print(name, R, level, "segments", len(seg), "NaN coordinates", int(np.isnan(seg).sum()), "reference", int(np.isnan(seg_r).sum()), "stats", stats)
        assert np.array_equal(offs, offs_r), (offs.tolist(), offs_r.tolist())
        assert keys.shape == keys_r.shape and np.array_equal(keys, keys_r)
        assert seg.shape == seg_r.shape and same_bits(seg, seg_r), np.argwhere(~((seg.view(np.uint32) == seg_r.view(np.uint32)) | (np.isnan(seg) & np.isnan(seg_r))))[:5]
        assert np.array_equal(np.isnan(seg), np.isnan(seg_r)), "NaN exactly where the formula gives NaN"
        got[level] = (seg, keys, offs)
    assert same_bits(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1]) and np.array_equal(got[0][2], got[2][2])
    if name in nf.MIXED:
        assert np.isnan(seg_r).any() and np.isfinite(seg_r).any()
    # the chaining works on the keys alone: it returns, and equals the plain chaining of the same segments
    for l in range(len(nf.Z)):
        k = keys_r[offs_r[l]:offs_r[l + 1]]
        order, lo, closed = impli.slice_loops(k)
        ro, rf, rc = np_slice.loops(k)
        assert np.array_equal(order, ro) and np.array_equal(lo, rf) and np.array_equal(closed, rc)
        assert np.array_equal(np.sort(order), np.arange(len(k)))


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", nf.DEPTHS)
@pytest.mark.parametrize("name", nf.NAMES)
def test_bounds_equal_the_plain_descent_and_hold_every_solid_sample(impli, oracle, name, depth):
    S = np.array(nf.BOX, np.float32)
    found_r, box_r, info = np_bounds.descent(impli, nf.TREES[name], S, depth)
    got = {}
    for level in LEVELS:
        found, box, stats = _at(impli, level, impli.bounds, nf.TREES[name], S, depth)
        print(name, depth, level, box.tolist(), stats, info)
        assert found and found_r and same_bits(box, box_r) and np.isfinite(box).all(), (box, box_r)
        got[level] = box
    assert same_bits(got[0], got[2])
    fitted = impli.fit_box(S, box_r, 32, 2)
    assert same_bits(fitted, np_bounds.fit_box(S, box_r, 32, 2))
    # the cells of the edge table whose sample (the cell's mid) is solid in the reference, NaN ones included
    F = nf.mass_field(oracle, name, depth)
    M = np_mass.mids(nf.BOX, depth)
    with np.errstate(invalid="ignore"):
        k, j, i = np.nonzero(~(F < 0))
    assert len(i) > 0
    for a, idx in enumerate((i, j, k)):
        assert M[a][idx].min() >= box_r[2 * a] and M[a][idx].max() <= box_r[2 * a + 1], (name, "axis", a, box_r.tolist())


# ---- rays ------------------------------------------------------------------------------------------------------------------------
def _seg_hi(impli, name, case):
    key = ("seg_hi", case.key)
    if key not in _CACHE:
        _CACHE[key] = _intervals(impli, name, edges.segment_boxes(case))[0][:, 1].reshape(len(case), edges.nseg(case.N))
    return _CACHE[key]


def _raycast_both_levels(impli, oracle, case, B):
    want = edges.reference(oracle, case, B)
    got = {}
    for level in LEVELS:
        got[level] = _at(impli, level, impli.raycast, *case.args(B), return_stats=True)
        print(case.key, "B", B, "level", level, "hits", int((want[0] >= 0).sum()), "NaN f", int(np.isnan(want[2]).sum()), "stats", got[level][4])
        tg._check_bits(impli, got[level], want, case.o, case.d, case.N)
        assert np.array_equal(np.isnan(got[level][2]), np.isnan(want[2])) and np.array_equal(np.isnan(got[level][3]), np.isnan(want[3]))
    for k in range(4):
        assert same_bits(got[0][k], got[2][k])
    assert got[0][4][1] == 0 and got[0][4][2] == tg._level0_segments(want[0], case.N)
    return want, got


@pytest.mark.parametrize("name", nf.NAMES)
def test_rays_equal_the_restatement(impli, oracle, name):
    case = nf.ray_case(name, 130)
    F = nf.ray_field(oracle, case)
    for B in nf.ROUNDS:
        want, got = _raycast_both_levels(impli, oracle, case, B)
    if "nan" in nf.CLAIMS[name]:
        rh, rt, rf, rn = want
        on_nan = (rh >= 1) & np.isnan(F[np.arange(len(case)), np.maximum(rh, 0)])
        assert on_nan.sum() >= 3 and np.isnan(rf[on_nan]).all() and np.isnan(got[2][2][on_nan]).all(), "bisections whose solid end is a NaN sample"
        assert (rt[on_nan] <= case.ts[rh[on_nan]]).all()


@pytest.mark.parametrize("name", nf.NAMES)
def test_spans_equal_the_restatement(impli, oracle, name):
    case = nf.ray_case(name, 130)
    F = nf.ray_field(oracle, case)
    n = len(case)
    for B in nf.ROUNDS:
        want = spans_in.reference(impli, oracle, case, B)
        got = {}
        for level in LEVELS:
            got[level] = _at(impli, level, impli.ray_spans, *case.args(B), want_normals=True, return_stats=True)
            print(name, "B", B, "level", level, "spans", int(want[0][-1]), "stats", got[level][5])
            ts_._check_bits(got[level], want, n, case.N)      # the stats identity outside + solid + evaluated == segments is in there
            st = got[level][5]
            assert st[1] + st[2] + st[3] == st[0] == n * edges.nseg(case.N)
            assert np.array_equal(np.isnan(got[level][3]), np.isnan(want[3])) and np.array_equal(np.isnan(got[level][4]), np.isnan(want[4]))
        assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1])
        for i in (2, 3, 4):
            assert same_bits(got[0][i], got[2][i])
    if name in nf.MIXED and name != "inter":
        offs, k = want[0], want[1]
        ray = np.repeat(np.arange(n), np.diff(offs))
        assert (np.isnan(F[ray, k[:, 0]]) & np.isfinite(F[ray, k[:, 1] - 1])).any(), "a span that opens on a NaN sample and closes on a finite one"


@pytest.mark.parametrize("name", nf.LATE_NAMES)
def test_a_nan_entry_in_the_second_march_batch(impli, oracle, name):
    case = nf.late_case(name)
    F = nf.ray_field(oracle, case)
    want, got = _raycast_both_levels(impli, oracle, case, 24)
    late = want[0] > 4096
    assert late.sum() >= 2 and np.isnan(F[np.arange(len(case)), np.maximum(want[0], 0)][late]).all() and np.isnan(got[2][2][late]).all()
    wants = spans_in.reference(impli, oracle, case, 24)
    for level in LEVELS:
        ts_._check_bits(_at(impli, level, impli.ray_spans, *case.args(24), want_normals=True, return_stats=True), wants, len(case), case.N)
    if name == "cone":
        _outside_in_front_of_nan(impli, name, case, F)
        assert got[2][4][1] > 0, "and the march kernel skips segments"


def _outside_in_front_of_nan(impli, name, case, F):
    """a segment the bound proves outside directly in front of one that holds NaN samples"""
    hi = _seg_hi(impli, name, case)
    nan_seg = np.array([[bool(np.isnan(F[r, 64 * j + 1:min(64 * j + 64, case.N) + 1]).any()) for j in range(edges.nseg(case.N))] for r in range(len(case))])
    with np.errstate(invalid="ignore"):
        print(case.key, "proved outside", int((hi < 0).sum()), "of", hi.size, "segments; in front of NaN samples", int(((hi[:, :-1] < 0) & nan_seg[:, 1:]).sum()))
        assert ((hi[:, :-1] < 0) & nan_seg[:, 1:]).any()
        assert not ((hi < 0) & nan_seg).any()


def test_a_proved_outside_segment_in_front_of_nan_samples_at_130(impli, oracle):
    case = nf.ray_case("cone", 130)
    _outside_in_front_of_nan(impli, "cone", case, nf.ray_field(oracle, case))


def test_span_chunks_give_the_same_bits(impli, oracle, monkeypatch):
    case = nf.ray_case("shear", 130)
    want = spans_in.reference(impli, oracle, case, 24)
    one = impli.ray_spans(*case.args(24), want_normals=True, return_stats=True)
    monkeypatch.setenv("IMPLISOLID_SPAN_CHUNK", "50")
    many = impli.ray_spans(*case.args(24), want_normals=True, return_stats=True)
    monkeypatch.delenv("IMPLISOLID_SPAN_CHUNK")
    assert one[5][7] == 1 and many[5][7] == (len(case) + 49) // 50
    ts_._check_bits(one, want, len(case), case.N)
    ts_._check_bits(many, want, len(case), case.N)
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1]) and all(same_bits(one[i], many[i]) for i in (2, 3, 4))
    assert many[5][:7] == one[5][:7]
