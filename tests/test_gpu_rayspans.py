"""Every solid span along a ray (implisolid_ray_spans) on the GPU.

The reference is tests/np_rayspans.py's restatement of the definition on field values that do not come from
the ray kernels (the oracle's, or ImplicitService.eval / np_sdf3d.evaluate for the sdf_3d shapes), with
np_normals.normals_ref at the returned ends.  offsets and k are integers and t, f and the normals are floats
the definition fixes bit for bit, whatever the pruning level proves and however the rays are chunked: every
comparison is an integer equality or same_bits.  The inputs are tests/rayspan_inputs.py's
(tests/test_cpu_rayspans.py asserts what they hold).

What a case holds is asserted on the reference: rays with no span and with one, a start inside and an end
inside everywhere; rays with several spans from N = 64 on for the shapes a line can enter twice
(rayspan_inputs.SEVERAL: an ellipsoid holds at most one span a ray, and two samples at most one run).
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_raycast   # noqa: E402
import ray_edge_inputs as edges   # noqa: E402
import rayspan_inputs as inputs   # noqa: E402
import test_gpu_raycast as tg   # noqa: E402
from np_normals import same_bits   # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
NAMES = inputs.NAMES
SPHERE, BIG, AWAY = inputs.SPHERE, inputs.BIG, inputs.AWAY
T0 = inputs.T0
STEPS = [1, 64, 65, 130]
ROUNDS = [0, 1, 24]
BOXES_PER_CALL = 4096


def _source(name):
    return "sdf3d" if name == "sdf3d" else "oracle"


def _at_level(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.ray_spans(*a, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check_bits(got, want, n, N, normals=True):
    offs, k, t, f, nrm, stats = got
    ro, rk, rt, rf, rn = want
    S = int(ro[-1])
    assert offs.dtype == np.int64 and offs.shape == (n + 1,) and k.dtype == np.int32 and t.dtype == f.dtype == np.float32
    bad = np.flatnonzero(offs != ro)
    assert len(bad) == 0, ("first differing offsets", bad[:5].tolist(), offs[bad[:5]].tolist(), ro[bad[:5]].tolist())
    assert k.shape == t.shape == f.shape == (S, 2)
    bad = np.flatnonzero((k != rk).any(1))
    assert len(bad) == 0, ("first differing spans", bad[:5].tolist(), k[bad[:5]].tolist(), rk[bad[:5]].tolist())
    assert same_bits(t, rt), np.flatnonzero((t.view(np.uint32) != rt.view(np.uint32)).any(1))[:5]
    assert same_bits(f, rf), np.flatnonzero((f.view(np.uint32) != rf.view(np.uint32)).any(1))[:5]
    if normals:
        assert nrm.shape == (S, 2, 3) and same_bits(nrm, rn), np.flatnonzero((nrm.view(np.uint32) != rn.view(np.uint32)).any((1, 2)))[:5]
    else:
        assert nrm is None
    count = np.diff(ro)
    nseg = inputs.nseg(N)
    assert stats[0] == n * nseg and stats[1] + stats[2] + stats[3] == stats[0], "the whole ray is walked"
    assert stats[4] == S and stats[5] == int((count > 0).sum())
    assert stats[6] == int((rk[ro[:-1][count > 0], 0] == 0).sum())


# ---- against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", STEPS)
@pytest.mark.parametrize("name", NAMES)
def test_spans_equal_the_restatement(impli, oracle, name, N):
    rays = inputs.suite(impli, oracle, name, N)
    n = len(rays)
    for B in ROUNDS:
        want = inputs.reference(impli, oracle, rays, B, _source(name))
        ro, rk = want[:2]
        count = np.diff(ro)
        assert (count == 0).any() and (count == 1).any(), "rays with no span and with one"
        assert rk[ro[0], 0] == 0 and rk[ro[1]].tolist() == [N, N + 1], "a start inside and an end inside"
        if N >= 64 and name in inputs.SEVERAL:
            assert (count >= 2).any(), "rays with several spans"
        if B == 24 and N > 1:
            ts = np_raycast.params(T0, rays.t1, N)
            moved_in = rk[:, 0] >= 1
            moved_out = rk[:, 1] <= N
            assert (want[2][moved_in, 0] < ts[rk[moved_in, 0]]).any() and (want[2][moved_out, 1] > ts[rk[moved_out, 1] - 1]).any(), \
                "the bisection moves entries down and exits up"
        for level in (0, 2):
            for normals in (True, False) if B == 24 else (B == 0,):
                got = _at_level(impli, level, *rays.args(B), want_normals=normals)
                print(name, N, B, level, "spans", int(ro[-1]), "stats", got[5])
                _check_bits(got, want, n, N, normals)
                assert got[5][7] == 1
                if level == 0:
                    assert got[5][1] == 0 and got[5][2] == 0 and got[5][3] == got[5][0]


# ---- consistency with the first-hit query -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["csg", "shell", "sdf3d"])
def test_the_first_span_s_entry_is_raycast_s_hit(impli, oracle, name):
    rays = inputs.suite(impli, oracle, name, 130)
    for B in (0, 24):
        hit, t, f, nrm = impli.raycast(*rays.args(B))
        offs, k, st, sf, sn = impli.ray_spans(*rays.args(B), want_normals=True)
        count = np.diff(offs)
        assert np.array_equal(hit < 0, count == 0), "a miss iff no span"
        first = offs[:-1][count > 0]
        assert (hit >= 0).any() and np.array_equal(k[first, 0], hit[hit >= 0])
        assert same_bits(st[first, 0], t[hit >= 0]) and same_bits(sf[first, 0], f[hit >= 0]) and same_bits(sn[first, 0], nrm[hit >= 0])


# ---- segment and batch boundaries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [0, 24])
@pytest.mark.parametrize("which", ["sphere", "two"])
def test_entries_and_exits_on_segment_and_batch_boundaries(impli, oracle, which, B):
    rays = inputs.placed_case(which)
    want = inputs.reference(impli, oracle, rays, B)
    ro, rk = want[:2]
    N, ks = rays.N, inputs.PLACED_KS
    for i, K in enumerate(ks):
        assert rk[ro[i + 1] - 1, 0] == K and rk[ro[len(ks) + i + 1] - 1, 1] == K, "the placed entry and exit"
    assert (rk[:, 1] == N + 1).any() and ((rk[:, 0] <= 4096) & (rk[:, 1] >= 4098) & (rk[:, 1] <= N)).any(), \
        "a ray that ends inside; a span across the batch boundary that closes before N"
    got = {}
    for level in (0, 2):
        got[level] = _at_level(impli, level, *rays.args(B), want_normals=True)
        print(which, B, level, "stats", got[level][5])
        _check_bits(got[level], want, len(rays), N)
    assert got[2][5][1] > 0 and got[2][5][2] > 0, "segments proved outside and proved solid"


def _bounds(impli, rays):
    """(lo, hi) (n, nseg) of the interval interpreter's bounds on the rays' segment boxes"""
    boxes = edges.segment_boxes(rays).reshape(-1, 6)
    iv = np.concatenate([impli.debug_intervals(rays.shape, boxes[i:i + BOXES_PER_CALL])[0] for i in range(0, len(boxes), BOXES_PER_CALL)])
    return iv[:, 0].reshape(len(rays), -1), iv[:, 1].reshape(len(rays), -1)


# ---- exact work ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sphere", "two"])
def test_the_proved_segments_are_the_ones_the_bounds_prove(impli, oracle, which):
    rays = inputs.placed_case(which)
    want = inputs.reference(impli, oracle, rays, 16)
    lo, hi = _bounds(impli, rays)
    assert np.isfinite(edges.segment_boxes(rays)).all()
    with np.errstate(invalid="ignore"):
        out, solid = hi < 0, lo >= 0
    assert not (out & solid).any()
    mixed = ~out & ~solid
    assert (mixed[:, 1:] & out[:, :-1]).any(), "a mixed segment directly behind a proved-outside one"
    assert (mixed[:, 1:] & solid[:, :-1]).any(), "a mixed segment directly behind a proved-solid one"
    n_seg = len(rays) * inputs.nseg(rays.N)
    got2 = _at_level(impli, 2, *rays.args(16))
    got0 = _at_level(impli, 0, *rays.args(16))
    print(which, "level 2", got2[5], "level 0", got0[5], "bounds: outside", int(out.sum()), "solid", int(solid.sum()))
    _check_bits(got2, want, len(rays), rays.N, False)
    _check_bits(got0, want, len(rays), rays.N, False)
    assert got2[5][:4] == [n_seg, int(out.sum()), int(solid.sum()), int(mixed.sum())]
    assert got0[5][:4] == [n_seg, 0, 0, n_seg]
    assert got0[5][4:7] == got2[5][4:7]


# ---- BIG and AWAY ------------------------------------------------------------------------------------------------------
def test_inside_everywhere_every_segment_is_proved_and_f_is_still_the_field(impli, oracle):
    o, d = tg._rays([0, 0, 0])
    n, N = len(o), 130
    fn = tg._field_fn(impli, oracle, "big", BIG)
    ts = np_raycast.params(0.0, 3.0, N)
    F = np.stack([fn(np_raycast.points(o, d, np.full(n, ts[0], f32))), fn(np_raycast.points(o, d, np.full(n, ts[N], f32)))], 1)
    for level in (0, 2):
        offs, k, t, f, nrm, stats = _at_level(impli, level, BIG, o, d, 0.0, 3.0, N, 8, want_normals=True)
        assert np.array_equal(offs, np.arange(n + 1)) and (k == [0, N + 1]).all() and (t == [ts[0], ts[N]]).all()
        assert same_bits(f, F), "the field at ts[0] and ts[N]"
        pts = np_raycast.points(np.repeat(o, 2, 0), np.repeat(d, 2, 0), t.reshape(-1))
        assert same_bits(nrm.reshape(-1, 3), tg._normals_at(impli, oracle, "big", BIG, pts))
        assert stats == ([n * 3, 0, n * 3, 0, n, n, n, 1] if level else [n * 3, 0, 0, n * 3, n, n, n, 1])


def test_rays_away_from_the_solid_evaluate_nothing(impli):
    o, d = tg._rays([0, 0, 0])
    n = len(o)
    offs, k, t, f, nrm, stats = impli.ray_spans(AWAY, o, d, T0, 3.5, 130, 8, want_normals=True, return_stats=True)
    assert not offs.any() and k.shape == (0, 2) and nrm.shape == (0, 2, 3)
    assert stats == [n * 3, n * 3, 0, 0, 0, 0, 0, 1]


def test_the_scratch_budget_cuts_the_chunks(impli, oracle):
    # 1024 segments a ray: 2^23 segment words hold 8192 rays
    n, N = 8193, 65536
    o, d = tg._rays([0, 0, 0], n=n)
    offs, k, t, f, nrm, stats = impli.ray_spans(BIG, o, d, 0.0, 3.0, N, 4, return_stats=True)
    assert stats == [n * 1024, 0, n * 1024, 0, n, n, n, 2]
    assert np.array_equal(offs, np.arange(n + 1)) and (k == [0, N + 1]).all() and (t == [0.0, 3.0]).all()
    fn = tg._field_fn(impli, oracle, "big", BIG)
    assert same_bits(f[:, 0], fn(o)) and same_bits(f[:, 1], fn(np_raycast.points(o, d, np.full(n, 3.0, f32))))


# ---- -0.0 is solid -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
def test_negative_zero_samples_are_solid(impli, level):
    rays, zeros = inputs.zero_rays()
    assert np.array_equal(rays.ts, np.arange(32, dtype=f32) * f32(0.0625))
    for B in (0, 3):
        want = inputs.reference(impli, None, rays, B, "np_sdf3d", normals=False)
        ro, rk, rt, rf, _ = want
        single = rk[:, 1] - rk[:, 0] == 1
        on_zero = (rf == 0) & np.signbit(rf)
        if B == 0:
            assert single.sum() >= 1000 and (np.diff(ro) >= 4).sum() >= 500, "many single-sample spans, many spans a ray"
            assert on_zero[:, 0].sum() >= 100 and on_zero[:, 1].sum() >= 100, "many spans open and close on a -0.0 sample"
        got = _at_level(impli, level, *rays.args(B))
        print("level", level, "B", B, "spans", int(ro[-1]), "single", int(single.sum()), "stats", got[5])
        _check_bits(got, want, len(rays), rays.N, False)


# ---- ray counts, chunks, reruns, the root matrix ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_ray_counts(impli, oracle, n):
    full = inputs.suite(impli, oracle, "csg", 130)
    rays = inputs.Rays(("suite", "csg", 130, n), full.shape, full.o[:n], full.d[:n], full.t0, full.t1, 130)
    want = inputs.reference(impli, oracle, rays, 24)
    assert want[0][-1] >= 1
    for level in (0, 2):
        _check_bits(_at_level(impli, level, *rays.args(24), want_normals=True), want, n, 130)


@pytest.mark.parametrize("n", [2049, 4097])
def test_ray_counts_across_the_scan_s_blocks(impli, oracle, n):
    # 2049: more than one 1024-lane pass of the single-block scan; 4097: the tiled scan's second tile
    o, d = tg._rays([0, 0, 0], n=n)
    rays = inputs.Rays(("many", n), SPHERE, o, d, T0, 3.5, 130)
    want = inputs.reference(impli, oracle, rays, 3, normals=False)
    count = np.diff(want[0])
    assert (count[2048:] > 0).any() and (count == 0).any()
    for level in (0, 2):
        _check_bits(_at_level(impli, level, *rays.args(3)), want, n, 130, False)


@pytest.mark.parametrize("name", ["two", "tree_deep"])
def test_chunks_give_the_same_bits_and_global_offsets(impli, oracle, name, monkeypatch):
    rays = inputs.suite(impli, oracle, name, 130)
    n = len(rays)
    want = inputs.reference(impli, oracle, rays, 24)
    one = impli.ray_spans(*rays.args(24), want_normals=True, return_stats=True)
    monkeypatch.setenv("IMPLISOLID_SPAN_CHUNK", "100")
    three = impli.ray_spans(*rays.args(24), want_normals=True, return_stats=True)
    monkeypatch.setenv("IMPLISOLID_SPAN_CHUNK", "1")
    m = 70
    single = impli.ray_spans(rays.shape, rays.o[:m], rays.d[:m], rays.t0, rays.t1, 130, 24, want_normals=True, return_stats=True)
    monkeypatch.delenv("IMPLISOLID_SPAN_CHUNK")
    assert one[5][7] == 1 and three[5][7] == 3 and single[5][7] == m
    _check_bits(one, want, n, 130)
    _check_bits(three, want, n, 130)
    assert three[5][:7] == one[5][:7]
    S = int(one[0][m])
    assert np.array_equal(single[0], one[0][:m + 1]) and np.array_equal(single[1], one[1][:S])
    for i in (2, 3, 4):
        assert same_bits(single[i], one[i][:S])
    assert (np.diff(one[0])[100:200] > 0).any() and one[0][100] > 0, "the later chunks hold spans at offsets above 0"


def test_two_calls_give_identical_bits(impli, oracle):
    rays = inputs.suite(impli, oracle, "tree_deep", 130)
    a = impli.ray_spans(*rays.args(24), want_normals=True, return_stats=True)
    # another shape and size in between: nothing of it may stay behind in the scratch or in the slot
    impli.ray_spans(BIG, rays.o[:70], rays.d[:70], 0.0, 3.0, 65, 3)
    b = impli.ray_spans(*rays.args(24), want_normals=True, return_stats=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(same_bits(a[i], b[i]) for i in (2, 3, 4)) and a[5] == b[5]
    _check_bits(b, inputs.reference(impli, oracle, rays, 24), len(rays), 130)


@pytest.mark.parametrize("level", [0, 2])
def test_ignore_root_matrix(impli, oracle, level):
    full = inputs.suite(impli, oracle, "csg", 130)
    moved = dict(full.shape, matrix=[1, 0, 0, 0.3, 0, 1, 0, -0.2, 0, 0, 1, 0.1])
    plain = inputs.Rays(("root", "plain"), full.shape, full.o, full.d, T0, 3.5, 130)
    rays = inputs.Rays(("root", "moved"), moved, full.o, full.d, T0, 3.5, 130)
    base = inputs.reference(impli, oracle, plain, 8)
    kept = inputs.reference(impli, oracle, rays, 8)
    rays_i = inputs.Rays(("root", "ignored"), moved, full.o, full.d, T0, 3.5, 130)
    want = inputs.reference(impli, oracle, rays_i, 8, ignore_root_matrix=True)
    assert np.array_equal(want[1], base[1]) and same_bits(want[2], base[2]) and not np.array_equal(kept[0], base[0]), "the root matrix moves the solid"
    _check_bits(_at_level(impli, level, *rays.args(8), want_normals=True, ignore_root_matrix=True), want, len(rays), 130)
    _check_bits(_at_level(impli, level, *rays.args(8), want_normals=True), kept, len(rays), 130)


# ---- views --------------------------------------------------------------------------------------------------------------------
def test_xray_view(impli):
    W, H, N, B = 33, 17, 100, 16
    view = dict(eye=(0, 0, 2), target=(0, 0, 0), up=(0, 1, 0), width=W, height=H)
    thick, count, stats = impli.xray_view(SPHERE, t0=0.5, t1=3.0, steps=N, bisect=B, ortho_height=2.0, return_stats=True, **view)
    assert thick.dtype == np.float64 and thick.shape == (H, W) and count.dtype == np.int32 and count.shape == (H, W)
    o, d = impli.view_rays(ortho_height=2.0, **view)
    offs, k, t, f, _ = impli.ray_spans(SPHERE, o, d, 0.5, 3.0, N, B)
    length, cnt = impli.span_lengths(offs, t, d)
    assert np.array_equal(thick.reshape(-1), length) and np.array_equal(count.reshape(-1), cnt) and stats[4] == offs[-1]
    # the centre ray crosses the sphere of radius 1/2 through its centre: both ends from the solid side
    ulps = 8 * float(np.spacing(f32(3.0)))
    c = thick[H // 2, W // 2]
    assert count[H // 2, W // 2] == 1 and 1.0 - 2 * (2.5 / N) * 2.0 ** -B - 2 * ulps <= c <= 1.0 + 2 * ulps, c
    assert count[0, 0] == 0 and thick[0, 0] == 0
    assert 0 < (count > 0).sum() < W * H and (count <= 1).all()
    pt, pc = impli.xray_view(SPHERE, t0=0.5, t1=3.0, steps=N, bisect=B, fov_y=0.7, **view)
    assert pc[H // 2, W // 2] == 1 and abs(pt[H // 2, W // 2] - 1.0) <= 2 * (2.5 / N) * 2.0 ** -B + 2 * ulps and pc[0, 0] == 0


def test_kernel_times(impli):
    o, d = tg._rays([0, 0, 0])
    impli.ray_spans_kernel_ms(True)
    try:
        impli.ray_spans(SPHERE, o, d, T0, 3.5, 130, 8)
        ms = impli.ray_spans_kernel_ms(True)
    finally:
        impli.ray_spans_kernel_ms(False)
    print("march, emit, refine ms", ms)
    assert len(ms) == 3 and all(v > 0 for v in ms)


# ---- errors -------------------------------------------------------------------------------------------------------------------
O1 = np.array([[0, 0, 2]], f32)
D1 = np.array([[0, 0, -1]], f32)


@pytest.mark.parametrize("kw", tg.BAD)
def test_bad_input_is_an_error(impli, kw):
    with pytest.raises(impli.ImplisolidError) as e:
        impli.ray_spans(kw.get("shape", SPHERE), kw.get("o", O1), kw.get("d", D1), kw.get("t0", 0.5), kw.get("t1", 3.0),
                        kw.get("steps", 64), kw.get("bisect", 8))
    assert str(e.value), "with a message"
    offs, k, t, f, _ = impli.ray_spans(SPHERE, O1, D1, 0.5, 3.0, 64, 8)
    assert offs.tolist() == [0, 1] and k[0, 0] >= 1 and k[0, 1] <= 64, "and the next call works"


def test_too_many_rays_are_refused_before_an_array_is_read(impli):
    fp, lp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    offs = np.zeros(2, np.int64)
    rc = impli.lib().implisolid_ray_spans(json.dumps(SPHERE).encode(), 0, O1.ctypes.data_as(fp), D1.ctypes.data_as(fp), (1 << 24) + 1,
                                          0.5, 3.0, 64, 8, 0, offs.ctypes.data_as(lp), None)
    assert rc == -1 and "2^24" in impli.last_error()
    assert impli.ray_spans(SPHERE, O1, D1, 0.5, 3.0, 64, 8)[0].tolist() == [0, 1], "and the next call works"


def test_normals_the_call_did_not_compute_are_refused(impli):
    fp = ctypes.POINTER(ctypes.c_float)
    impli.ray_spans(SPHERE, O1, D1, 0.5, 3.0, 64, 8, want_normals=False)
    k, t, f, nrm = np.zeros(2, np.int32), np.zeros(2, f32), np.zeros(2, f32), np.zeros(6, f32)
    L = impli.lib()
    assert L.implisolid_ray_spans_copy(k.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), t.ctypes.data_as(fp), f.ctypes.data_as(fp),
                                       nrm.ctypes.data_as(fp)) == -1 and "no normals" in impli.last_error()
    assert L.implisolid_ray_spans_copy(k.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), t.ctypes.data_as(fp), f.ctypes.data_as(fp), None) == 0
    assert k[0] >= 1 and t[0] < t[1], "the result is still there"
