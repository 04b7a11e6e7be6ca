"""Host side of the ray cast (implisolid_ray_params, view_rays, ray_points) against the restatement
tests/np_raycast.py, the restatement's own rule against an analytic sphere, and the inputs of
tests/test_gpu_raycast_edges.py.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_raycast   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("implisolid_raycast", "implisolid_ray_params")
DYADIC = (0.5, 4.5)
NON_DYADIC = (0.3, 3.7)
f32 = np.float32


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_abi_declares_the_ray_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for name in NAMES + ("implisolid_debug_raycast_ms",):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and ("int %s(" % name) in header, name


# ---- ray_params ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("rng", [DYADIC, NON_DYADIC])
def test_params_equal_the_restatement(impli, rng, N):
    ts = impli.ray_params(rng[0], rng[1], N)
    ref = np_raycast.params(rng[0], rng[1], N)
    assert ts.dtype == np.float32 and ts.shape == (N + 1,)
    assert np.array_equal(_u32(ts), _u32(ref))
    assert ts[0] == f32(rng[0]) and ts[N] == f32(rng[1])
    assert (ts[:-1] <= ts[1:]).all()


def test_non_dyadic_params_round(impli):
    # the case is not blind: the separately rounded product differs from the float64 formula somewhere
    ts = impli.ray_params(NON_DYADIC[0], NON_DYADIC[1], 1000)
    exact = (np.float64(f32(NON_DYADIC[0])) + np.arange(1001) * ((np.float64(f32(NON_DYADIC[1])) - np.float64(f32(NON_DYADIC[0]))) / 1000))
    assert (ts != exact.astype(np.float32)).any()


@pytest.mark.parametrize("t0, t1, N", [(1.0, 1.0, 8), (2.0, 1.0, 8), (0.0, np.inf, 8), (np.nan, 1.0, 8), (-np.inf, 0.0, 8),
                                       (0.0, 1.0, 0), (0.0, 1.0, 65537), (-3e38, 3e38, 8)])
def test_bad_ranges_and_steps_are_refused_with_a_message(impli, t0, t1, N):
    L = impli.lib()
    ts = np.zeros(70000, np.float32)
    assert L.implisolid_ray_params(t0, t1, N, ts.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == -1
    assert impli.last_error()
    with pytest.raises(impli.ImplisolidError) as e:
        impli.ray_params(t0, t1, N)
    assert str(e.value), "with a message"
    assert impli.ray_params(0, 1, 4).tolist() == [0, 0.25, 0.5, 0.75, 1], "and the next call works"


def test_a_table_that_would_decrease_is_refused(impli):
    # a range a few ulps wide: where the restatement's ts[N - 1] exceeds t1 the host must refuse, else accept
    seen = set()
    for ulps in range(1, 40):
        t0 = f32(1000)
        t1 = (t0.view(np.uint32) + np.uint32(ulps)).view(np.float32)
        for N in (3, 7, 64, 1000):
            ref = np_raycast.params(t0, t1, N)
            ok = bool((ref[:-1] <= ref[1:]).all())
            assert (ref[:-2] <= ref[1:-1]).all(), "only the last entry can violate the order"
            seen.add(ok)
            if ok:
                assert np.array_equal(_u32(impli.ray_params(t0, t1, N)), _u32(ref))
            else:
                with pytest.raises(impli.ImplisolidError):
                    impli.ray_params(t0, t1, N)
    assert True in seen
    print("cases refused:", False in seen)


# ---- ray_points ---------------------------------------------------------------------------------------------
def test_ray_points_round_like_the_restatement(impli):
    rng = np.random.default_rng(3)
    o = rng.uniform(-2, 2, (100, 3)).astype(f32)
    d = rng.uniform(-1, 1, (100, 3)).astype(f32)
    t = rng.uniform(0, 4, 100).astype(f32)
    p = impli.ray_points(o, d, t)
    assert p.dtype == np.float32 and p.shape == (100, 3)
    assert np.array_equal(_u32(p), _u32(np_raycast.points(o, d, t)))
    fused = (o.astype(np.float64) + t[:, None].astype(np.float64) * d.astype(np.float64)).astype(f32)
    assert (p != fused).any(), "the product is rounded before the sum"
    assert np.array_equal(_u32(impli.ray_points(o, d, 0.5)), _u32(np_raycast.points(o, d, np.full(100, 0.5, f32))))
    with pytest.raises(impli.ImplisolidError):
        impli.ray_points(o, d[:5], t)


# ---- the restatement against an analytic sphere --------------------------------------------------------------
def _sphere(p):
    p = np.asarray(p, f32)
    return (f32(1) - (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]) / f32(0.25)).astype(f32)


def _centre_rays(n=50, seed=1):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = (2.0 * v).astype(f32)                       # on the sphere of radius 2
    d = (-v).astype(f32)                            # unit, through the centre: the entry is at t = 1.5
    return o, d


@pytest.mark.parametrize("N", [64, 65, 130])
def test_cast_finds_the_analytic_entry(N):
    o, d = _centre_rays()
    t0, t1 = 0.25, 3.0
    ts = np_raycast.params(t0, t1, N)
    step = (t1 - t0) / N
    # float32 o and d: the entry distance of the ray as rounded, in float64
    od = (o.astype(np.float64) * d.astype(np.float64)).sum(1)
    dd = (d.astype(np.float64) ** 2).sum(1)
    oo = (o.astype(np.float64) ** 2).sum(1)
    entry = (-od - np.sqrt(od * od - dd * (oo - 0.25))) / dd
    assert np.abs(entry - 1.5).max() < 1e-5
    hit, t, f = np_raycast.cast(_sphere, o, d, ts, 0)
    ulps = 8 * np.spacing(f32(3.0))   # p(t), its squares and their sum round a few times at magnitudes up to 3
    assert (hit >= 1).all() and np.array_equal(t, ts[hit])
    assert (t >= entry - ulps).all() and (t - entry <= step + ulps).all(), "B = 0: within one step behind the entry"
    assert (np.abs(hit - np.ceil((entry - t0) / step)) <= 1).all()
    assert (~(f < 0)).all()
    hit20, t20, f20 = np_raycast.cast(_sphere, o, d, ts, 20)
    assert np.array_equal(hit20, hit)
    assert (t20 >= entry - ulps).all() and (t20 - entry <= step * 2.0 ** -20 + ulps).all(), "B = 20"
    assert (~(f20 < 0)).all() and np.array_equal(_u32(f20), _u32(_sphere(np_raycast.points(o, d, t20))))
    assert (t20 <= t).all()


def test_cast_inside_miss_and_zero_direction():
    ts = np_raycast.params(0.25, 3.0, 65)
    o = np.array([[0.1, 0, 0], [2, 2, 0], [0.2, 0.1, 0], [2, 0, 0], [2, 0, 0]], f32)
    d = np.array([[1, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0], [-2, 0, 0]], f32)
    hit, t, f = np_raycast.cast(_sphere, o, d, ts, 12)
    assert hit[0] == 0 and t[0] == ts[0] and f[0] == _sphere(np_raycast.points(o[:1], d[:1], ts[:1]))[0], "starts inside"
    assert hit[1] == -1 and t[1] == ts[-1] and f[1] == 0, "misses"
    assert hit[2] == 0 and hit[3] == -1, "an all-zero direction samples the origin"
    assert hit[4] >= 1 and abs(float(t[4]) - 0.75) <= (2.75 / 65) * 2.0 ** -12 + 1e-6, "a direction of length 2 halves t"


def test_cast_counts_negative_zero_and_nan_as_solid():
    vals = {0: np.array([-1, -1, -0.0, 1], f32), 1: np.array([-1, np.nan, -1, -1], f32), 2: np.array([-1, -1, -1, -1], f32)}
    o = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], f32)
    d = np.array([[0, 1, 0]] * 3, f32)
    ts = np_raycast.params(0, 3, 3)

    def field(p):
        return np.array([vals[int(q[0])][int(round(float(q[1])))] for q in p], f32)
    hit, t, f = np_raycast.cast(field, o, d, ts, 0)
    assert hit.tolist() == [2, 1, -1] and t.tolist() == [2, 1, 3]
    assert np.signbit(f[0]) and f[0] == 0 and np.isnan(f[1]) and f[2] == 0 and not np.signbit(f[2])


# ---- view_rays ----------------------------------------------------------------------------------------------
EYE, TARGET, UP = (2.0, 1.0, 0.5), (0.1, -0.2, 0.0), (0, 0, 1)


@pytest.mark.parametrize("kw", [dict(fov_y=0.8), dict(ortho_height=1.5)])
def test_view_rays(impli, kw):
    W, H = 33, 17
    o, d = impli.view_rays(EYE, TARGET, UP, W, H, **kw)
    assert o.dtype == np.float32 and d.dtype == np.float32 and o.shape == d.shape == (W * H, 3)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() <= 1e-6
    c = (H // 2) * W + W // 2
    fwd = np.subtract(TARGET, EYE)
    fwd /= np.linalg.norm(fwd)
    assert np.abs(d[c] - fwd).max() <= 1e-6 and np.abs(o[c] - np.asarray(EYE)).max() <= 1e-6, "the centre ray points at the target"
    O, Dm = o.reshape(H, W, 3).astype(np.float64), d.reshape(H, W, 3).astype(np.float64)
    if "ortho_height" in kw:
        assert np.abs(Dm - fwd).max() <= 1e-6
        # pixel centres: the rows span ortho_height (H - 1) / H, the columns the same scaled by the aspect
        assert abs(np.linalg.norm(O[0, 0] - O[-1, 0]) - 1.5 * (H - 1) / H) <= 1e-6
        assert abs(np.linalg.norm(O[0, 0] - O[0, -1]) - 1.5 * (W / H) * (W - 1) / W) <= 1e-6
        assert O[0, :, 2].min() > O[-1, :, 2].max(), "row 0 is the top row"
        assert np.abs((O - np.asarray(EYE)) @ fwd).max() <= 1e-6, "origins on the view plane"
    else:
        assert np.abs(O - np.asarray(EYE)).max() <= 1e-6
        top, bottom = Dm[0, W // 2], Dm[-1, W // 2]
        assert top[2] > bottom[2], "row 0 is the top row"
        # the centre column's outermost pixel centres are (H - 1) / H of the half angle's tangent apart
        assert abs(np.tan(np.arccos(np.clip(top @ fwd, -1, 1))) - np.tan(0.4) * (H - 1) / H) <= 1e-5


@pytest.mark.parametrize("kw", [dict(), dict(fov_y=0.8, ortho_height=1.5)])
def test_view_rays_take_exactly_one_projection(impli, kw):
    with pytest.raises(ValueError):
        impli.view_rays(EYE, TARGET, UP, 8, 8, **kw)


# ---- the inputs of tests/test_gpu_raycast_edges.py (tests/ray_edge_inputs.py) ---------------------------
# What the GPU tests rely on is asserted here on the oracle's field alone, so an edit that spoils an input
# fails without a GPU.
import ray_edge_inputs as edges   # noqa: E402


@pytest.mark.parametrize("N", edges.PLACED_N)
def test_placed_rays_hit_first_on_the_chosen_samples(oracle, N):
    case, ks = edges.placed_case(N), edges.placed_ks(N)
    assert len(case) == len(ks) + edges.MISSES <= 32
    assert {1, 64, 65, 4096, 4097, N - 1, N} <= set(ks.tolist()) and (N <= 8192 or {8192, 8193} <= set(ks.tolist()))
    for B in (0, 24):
        rh, rt, rf, _ = edges.reference(oracle, case, B, normals=False)
        assert np.array_equal(rh[:len(ks)], ks) and (rh[len(ks):] == -1).all()
        assert (~(rf[:len(ks)] < 0)).all() and (rt[:len(ks)] <= case.ts[ks]).all()
    # the samples in front of the hits are outside, and the hits lie in every batch the table has
    F = edges.sampled(oracle, case)
    assert (F[np.arange(len(ks)), ks - 1] < 0).all()
    assert set((edges.hit_segment(ks, N) // 64).tolist()) >= set(range(min((edges.nseg(N) + 63) // 64, 3))), "batches 0, 1 and 2"
    assert N % 64 != 0 or N == 65536, "the last segment is partial"


@pytest.mark.parametrize("name", edges.SEEDED_NAMES)
def test_seeded_rays_hit_in_both_batches_and_miss(oracle, name):
    case = edges.seeded_case(name)
    assert len(case) == edges.SEEDED_RAYS
    tree = oracle.mp5_to_nodes(json.dumps(case.shape), False)
    assert oracle.eval_implicit(tree, np.array([edges.SEEDED_INSIDE[name]], f32))[0] > 0
    rh = edges.reference(oracle, case, 24)[0]
    print(name, "beyond 4096:", int((rh > 4096).sum()), "up to 4096:", int(((rh >= 1) & (rh <= 4096)).sum()), "misses:", int((rh < 0).sum()))
    assert (rh > 4096).sum() >= 8 and ((rh >= 1) & (rh <= 4096)).sum() >= 8 and (rh < 0).sum() >= 8
    assert np.array_equal(rh, edges.reference(oracle, case, 0)[0])


def test_the_gap_rays_pass_one_sphere_and_hit_the_other(oracle):
    case = edges.gap_case()
    rh = edges.reference(oracle, case, 16)[0]
    assert rh.tolist() == edges.GAP_HITS == [2460, 6270, 6315, 6479, -1, 6326]
    assert edges.hit_segment(rh, case.N)[[0, 1, 2, 3, 5]].tolist() == [38, 97, 98, 101, 98]
    F = edges.sampled(oracle, case)
    # the ray at x = 0.26 passes the small sphere (z = 1: t = 2, sample 3280) at a field value of -0.082
    near = F[edges.GAP_PASS, 2800:3800]
    assert -0.09 < near.max() < -0.08 and near.max() == F[edges.GAP_PASS, :6000].max()
    # the oblique ray passes it at 0.2515 from its centre (t = 2.04, sample 2940): no sample of it is solid
    ob = F[edges.GAP_OBLIQUE, 2700:3200]
    assert -0.0125 < ob.max() < -0.0115 and (F[edges.GAP_OBLIQUE, :6326] < 0).all()
    # the same points with the directions halved and the range doubled: ts doubles exactly
    same = edges.gap_case("halved")
    assert np.array_equal(_u32(same.ts), _u32(f32(2) * case.ts))
    T = np.broadcast_to(case.ts[None, :], (len(case), case.N + 1))
    assert np.array_equal(_u32(np_raycast.points(case.o, case.d, T)), _u32(np_raycast.points(same.o, same.d, f32(2) * T)))
    assert edges.reference(oracle, same, 16)[0].tolist() == edges.GAP_HITS
    # t1 alone doubled: other samples of the same lines
    other = edges.reference(oracle, edges.gap_case("halved_t1"), 16)[0]
    assert (other > 4096).sum() == 4 and 1 <= other[0] <= 4096 and other[4] == -1 and other.tolist() != edges.GAP_HITS
    # the chunked rays: hits in both batches and misses, ten rays
    ch = edges.reference(oracle, edges.gap_chunk_case(), 16)[0]
    assert len(ch) == 10 and ((ch >= 1) & (ch <= 4096)).sum() >= 2 and (ch > 4096).sum() >= 2 and (ch < 0).sum() >= 1


@pytest.mark.parametrize("N", edges.OVERFLOW_N)
@pytest.mark.parametrize("name", edges.OVERFLOW_NAMES)
def test_the_first_overflowed_sample_is_a_nan_hit(oracle, name, N):
    case = edges.overflow_case(name, N)
    assert np.isfinite(case.ts).all() and np.isfinite(case.o).all() and np.isfinite(case.d).all()
    n = len(edges.OVERFLOW_DIRS)
    assert (case.d[:n] != 0).all() and ((case.d[:n] < 0).sum(axis=1) == 1).all()
    assert (np.abs(np.linalg.norm(case.d[:n].astype(np.float64), axis=1) - 4) < 0.25).all()
    over = edges.first_overflowed(case)
    F = edges.sampled(oracle, case)
    rh, rt, rf, rn = edges.reference(oracle, case, 24)
    print(name, N, "hits", rh.tolist(), "first overflowed", over.tolist(), "t", rt.tolist())
    assert (over[:n] >= 1).all() and np.array_equal(rh[:n], over[:n]), "the first solid sample is the first overflowed one"
    assert np.isnan(F[np.arange(n), rh[:n]]).all() and np.isnan(rf[:n]).all() and np.isnan(rn[:n]).all()
    assert (F[np.arange(n), rh[:n] - 1] < 0).all()
    # the components overflow at different samples: at the hit only some coordinates are infinite
    p = np_raycast.points(case.o[:n], case.d[:n], case.ts[rh[:n]])
    assert (np.isinf(p).sum(axis=1) < 3).any() and not np.isnan(p).any()
    # the bisection moves t between the last finite and the first overflowed point
    assert (rt[:n] < case.ts[rh[:n]]).all() and (rt[:n] > case.ts[rh[:n] - 1]).all()
    assert rh[n] == 0 and rf[n] > 0 and over[n] >= 1, "starts inside, and overflows later"
    assert rh[n + 1] == -1 and over[n + 1] == -1, "a zero direction never overflows"
    assert len(set(edges.hit_segment(rh[:n], N).tolist())) > 1 and (N < 4097 or (rh[:n] > 64).all())


def test_rays_that_start_behind_their_origin_hit_on_both_sides_of_zero(oracle):
    import test_gpu_raycast as tg
    o, d = tg._case(None, oracle, "twist")[:2]
    case = edges.behind_case(o, d)
    assert len(case) == tg.N_RAYS and (case.ts < 0).any() and (case.ts > 0).any()
    rh, rt, rf, _ = edges.reference(oracle, case, 24)
    print("t < 0:", int(((rh >= 1) & (rt < 0)).sum()), "t > 0:", int(((rh >= 1) & (rt > 0)).sum()), "misses:", int((rh < 0).sum()))
    assert ((rh >= 1) & (rt < 0)).sum() >= 8 and ((rh >= 1) & (rt > 0)).sum() >= 8 and (rh < 0).sum() >= 8


def test_segment_boxes_hold_their_samples():
    case = edges.gap_case()
    boxes = edges.segment_boxes(case)
    assert boxes.shape == (len(case), edges.nseg(case.N), 6) and boxes.dtype == np.float32
    T = np.broadcast_to(case.ts[None, :], (len(case), case.N + 1))
    p = np_raycast.points(case.o, case.d, T)
    for j in (0, 1, 63, 64, edges.nseg(case.N) - 1):
        q = p[:, 64 * j:min(64 * j + 64, case.N) + 1]
        assert (boxes[:, j, None, 0::2] <= q).all() and (q <= boxes[:, j, None, 1::2]).all()
        assert np.array_equal(boxes[:, j, 5], q[:, 0, 2]) and np.array_equal(boxes[:, j, 4], q[:, -1, 2]), "rays down z"
    assert edges.expected_work(np.array([[-1, -1, 1], [-1, -1, -1]], f32), np.array([130, -1]), 130) == (5, 1)
    with pytest.raises(AssertionError):
        edges.expected_work(np.full((1, 3), -1, f32), np.array([70]), 130)
