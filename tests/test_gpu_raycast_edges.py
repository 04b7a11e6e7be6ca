"""implisolid_raycast where tests/test_gpu_raycast.py is blind: rays of more than 64 segments (the march
kernel's second and later batches, up to the 1024 segments of N = 65536), hits on both sides of segment
and batch boundaries and on the last partial segment, the exact work figures at pruning level 2, a run
of skipped segments between a live one and the hit, sample points that overflow to infinity (a NaN
field, which is solid), t0 < 0, blocks with idle waves and chunks of three rays.

The inputs are tests/ray_edge_inputs.py's (tests/test_cpu_raycast.py asserts what they hold).  The
reference is np_raycast.cast of the oracle's field with np_normals.normals_ref at the returned points.
Every comparison is an integer equality or same_bits, at pruning levels 0 and 2.

The work figures: the march kernel bounds segment j of a ray over the box spanned by p(ts[64 j]) and
p(ts[min(64 j + 64, N)]) and skips it when the bound's upper end is negative.  debug_intervals runs the
same interval interpreter on boxes given by the caller (pinned by test_gpu_intervals.py), so the
segments skipped and evaluated up to the hit are known exactly without the ray kernels.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_raycast   # noqa: E402
import ray_edge_inputs as edges   # noqa: E402
from np_normals import same_bits   # noqa: E402
from test_gpu_raycast import _at_level, _case, _check_bits, _level0_segments   # noqa: E402

pytestmark = pytest.mark.gpu

BOXES_PER_CALL = 4096


def _bounds(impli, case):
    """(n, nseg) upper ends of the interval interpreter's bounds on the case's segment boxes, once per case"""
    def make():
        boxes = edges.segment_boxes(case).reshape(-1, 6)
        hi = [impli.debug_intervals(case.shape, boxes[i:i + BOXES_PER_CALL])[0][:, 1] for i in range(0, len(boxes), BOXES_PER_CALL)]
        return np.concatenate(hi).reshape(len(case), edges.nseg(case.N))
    return edges._cached(("hi", case.key), make)


def _run(impli, oracle, case, B, exact_work=True):
    """the case at both levels against the reference: bits, the exact work figures, and level 0 == level 2"""
    want = edges.reference(oracle, case, B)
    got = {}
    for level in edges.LEVELS:
        g = _at_level(impli, level, *case.args(B))
        print(case.key, "B", B, "level", level, "hits", int((want[0] >= 0).sum()), "stats", g[4])
        _check_bits(impli, g, want, case.o, case.d, case.N)
        assert g[4][5] == 1
        if level == 0:
            assert g[4][1] == 0 and g[4][2] == _level0_segments(want[0], case.N)
        elif exact_work:
            skipped, evaluated = edges.expected_work(_bounds(impli, case), want[0], case.N)
            print("   expected skipped", skipped, "evaluated", evaluated)
            assert (g[4][1], g[4][2]) == (skipped, evaluated)
        got[level] = g
    for k in range(4):
        assert same_bits(got[0][k], got[2][k])
    return want, got


# ---- 1. hits on chosen samples, across batches -----------------------------------------------------------
@pytest.mark.parametrize("B", [0, 24])
@pytest.mark.parametrize("N", edges.PLACED_N)
def test_hits_on_chosen_samples_of_every_batch(impli, oracle, N, B):
    case, ks = edges.placed_case(N), edges.placed_ks(N)
    want, got = _run(impli, oracle, case, B)
    assert np.array_equal(want[0][:len(ks)], ks) and (want[0][len(ks):] == -1).all()
    assert np.array_equal(got[2][0][:len(ks)], ks)
    # the rays that miss walk every segment at level 0: 1024 each at N = 65536
    walked = _level0_segments(want[0][:len(ks)], N) + edges.MISSES * edges.nseg(N)
    assert got[0][4][2] == walked and got[0][4][0] == len(case) * edges.nseg(N)
    # at level 2 a ray that misses is skipped whole, and pruning skips in every batch
    hi = _bounds(impli, case)
    assert (hi[len(ks):] < 0).all()
    far = int(np.flatnonzero(ks == N)[0])
    assert (hi[far, ::64][:-1] < 0).all() and got[2][4][1] >= edges.MISSES * edges.nseg(N) + edges.nseg(N) - 2


@pytest.mark.parametrize("name", edges.SEEDED_NAMES)
def test_seeded_rays_on_trees_with_modes_words(impli, oracle, name):
    case = edges.seeded_case(name)
    want, got = _run(impli, oracle, case, 24)
    rh = want[0]
    assert (rh > 4096).sum() >= 8 and ((rh >= 1) & (rh <= 4096)).sum() >= 8 and (rh < 0).sum() >= 8
    # the hit segments' modes words are not all 0: somewhere the bounds decide a CSG node
    boxes = edges.segment_boxes(case)[np.arange(len(case)), edges.hit_segment(rh, case.N)]
    _, modes = impli.debug_intervals(case.shape, boxes[rh >= 1])
    assert (modes != 0).any()
    assert got[2][4][1] > 0, "and some segments are skipped"
    _run(impli, oracle, case, 0)


# ---- 3. a gap between a live segment and the hit ---------------------------------------------------------------
def test_the_gap_case_has_a_live_segment_then_skipped_ones_then_the_hit(impli, oracle):
    """The axis-parallel ray at x = 0.26 has no such segment: a segment's box is the segment itself (x and y
    fixed), the bound follows the field (at most -0.082 there) to within its 2^-16 margin, and every segment
    before the hit's is proved outside.  The oblique ray's boxes are 0.008 wide and reach into the small
    sphere, which the ray passes at 0.0015 from its surface."""
    case = edges.gap_case()
    rh = edges.reference(oracle, case, 16)[0]
    assert rh.tolist() == edges.GAP_HITS
    hit_seg = edges.hit_segment(rh, case.N)
    out = _bounds(impli, case) < 0
    assert hit_seg[edges.GAP_PASS] == 97 and out[edges.GAP_PASS, :97].all() and not out[edges.GAP_PASS, 97]
    r = edges.GAP_OBLIQUE
    jh = int(hit_seg[r])
    assert jh == 98 and jh // 64 == 1, "the hit lies in the second batch"
    live = np.flatnonzero(~out[r, :jh])
    print("the oblique ray: live segments before the hit segment", live.tolist(), "skippable behind it", np.flatnonzero(out[r, jh:128]).tolist())
    assert len(live) >= 1 and live.max() < 64, "live segments near the small sphere, in the first batch"
    assert out[r, live.max() + 1:jh].all() and jh - live.max() > 32, "a run of skipped segments between them and the hit"
    assert out[r, 64:jh].all(), "the hit's batch starts with skipped segments"
    assert out[r, jh + 1:128].any(), "skippable segments behind the hit in the hit's batch"
    assert out[r, :live.min()].all(), "and the ray's first segments are skipped"


@pytest.mark.parametrize("B", [0, 16])
@pytest.mark.parametrize("which", sorted(edges.GAP_RANGES))
def test_pruning_resumes_after_a_gap(impli, oracle, which, B):
    case = edges.gap_case(which)
    want, got = _run(impli, oracle, case, B)
    if which != "halved_t1":
        assert want[0].tolist() == edges.GAP_HITS
    if which == "halved":
        base = edges.gap_case()
        unit = edges.reference(oracle, base, B)
        assert same_bits(np_raycast.points(case.o, case.d, want[1]), np_raycast.points(base.o, base.d, unit[1]))
        assert same_bits(want[2], unit[2]) and same_bits(want[3], unit[3]), "the same points: the same field and normals"
    assert got[2][4][1] > 0 and got[2][4][2] < got[0][4][2]


# ---- 4. overflowed sample points and NaN fields ------------------------------------------------------------------
@pytest.mark.parametrize("N", edges.OVERFLOW_N)
@pytest.mark.parametrize("name", edges.OVERFLOW_NAMES)
def test_overflowed_samples_are_solid(impli, oracle, name, N):
    case = edges.overflow_case(name, N)
    n = len(edges.OVERFLOW_DIRS)
    over = edges.first_overflowed(case)
    # the oracle and ImplicitService.eval agree at the overflowed points, the hits' among them
    k = np.clip(np.stack([over - 1, over, over + 1, np.full(len(case), N)], 1), 0, N)
    pts = np_raycast.points(case.o, case.d, case.ts[k]).reshape(-1, 3)
    with impli.ImplicitService(case.shape) as svc:
        assert same_bits(svc.eval(pts), edges.sampled(oracle, case)[np.arange(len(case))[:, None], k].reshape(-1))
    for B in (0, 24):
        want, got = _run(impli, oracle, case, B, exact_work=False)
        rh, rt, rf, rn = want
        assert np.array_equal(rh[:n], over[:n]) and np.isnan(rf[:n]).all() and np.isnan(rn[:n]).all()
        assert rh[n] == 0 and rh[n + 1] == -1
        assert np.isnan(got[2][2][:n]).all() and np.isnan(got[2][3][:n]).all()
        if B:
            assert (rt[:n] < case.ts[rh[:n]]).all(), "the bisection runs between finite and infinite points"


# ---- 5. small cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [0, 24])
def test_rays_that_start_behind_their_origin(impli, oracle, B):
    o, d = _case(impli, oracle, "twist")[:2]
    case = edges.behind_case(o, d)
    want, _ = _run(impli, oracle, case, B)
    rh, rt = want[:2]
    assert ((rh >= 1) & (rt < 0)).sum() >= 8 and ((rh >= 1) & (rt > 0)).sum() >= 8 and (rh < 0).sum() >= 8


@pytest.mark.parametrize("n", [2, 3, 5])
def test_blocks_with_idle_waves(impli, oracle, n):
    # hits beyond sample 4096, hits before it and a miss among the first five
    full = edges.seeded_case("csg")
    rh = edges.reference(oracle, full, 24)[0]
    order = np.concatenate([np.flatnonzero(rh > 4096)[:2], np.flatnonzero((rh >= 1) & (rh <= 4096))[:2], np.flatnonzero(rh < 0)[:1]])
    case = edges.Case(("seeded", "csg", "first", n), full.shape, full.o[order[:n]], full.d[order[:n]], full.t0, full.t1, full.N)
    want, _ = _run(impli, oracle, case, 24)
    assert np.array_equal(want[0], rh[order[:n]]) and want[0][0] > 4096


def test_chunks_of_three_rays_give_the_same_bits(impli, oracle, monkeypatch):
    case = edges.gap_chunk_case()
    want = edges.reference(oracle, case, 16)
    one = impli.raycast(*case.args(16), return_stats=True)
    monkeypatch.setenv("IMPLISOLID_RAY_CHUNK", "3")
    four = impli.raycast(*case.args(16), return_stats=True)
    monkeypatch.delenv("IMPLISOLID_RAY_CHUNK")
    print("one chunk", one[4], "chunks of three", four[4])
    assert one[4][5] == 1 and four[4][5] == 4
    _check_bits(impli, one, want, case.o, case.d, case.N)
    _check_bits(impli, four, want, case.o, case.d, case.N)
    assert four[4][:5] == one[4][:5]
    assert (one[4][1], one[4][2]) == edges.expected_work(_bounds(impli, case), want[0], case.N)
    for k in range(4):
        assert same_bits(four[k], one[k])
