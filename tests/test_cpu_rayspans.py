"""Host side of the solid spans along rays (implisolid_ray_spans): the ABI's declarations and refusals, the
restatement tests/np_rayspans.py against analytic solids, span_lengths, and the inputs of
tests/test_gpu_rayspans.py (tests/rayspan_inputs.py) asserted on the oracle's field alone.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_raycast   # noqa: E402
import np_rayspans   # noqa: E402
import rayspan_inputs as inputs   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
fp = ctypes.POINTER(ctypes.c_float)
lp = ctypes.POINTER(ctypes.c_int64)
EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
SPHERE = json.dumps({"type": "iellipsoid", "matrix": EYE}).encode()


def test_abi_declares_the_span_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for decl in ("int64_t implisolid_ray_spans(", "int implisolid_ray_spans_copy(", "int implisolid_debug_ray_spans_ms("):
        name = decl.split()[1][:-1]
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and decl in header, name
    for name in ("ray_spans", "span_lengths", "xray_view", "ray_spans_kernel_ms"):
        assert callable(getattr(impli, name))


# ---- refusals: nothing of these reaches a device --------------------------------------------------------------
def _call(L, shape=SPHERE, o=(0, 0, 2), d=(0, 0, -1), n=1, t0=0.5, t1=3.0, steps=64, bisect=8, offsets=True):
    oo, dd = np.array(o, f32), np.array(d, f32)
    offs = np.full(max(n, 0) + 1 if n < 100 else 2, 7, np.int64)
    rc = L.implisolid_ray_spans(shape, 0, oo.ctypes.data_as(fp), dd.ctypes.data_as(fp), n, t0, t1, steps, bisect, 0,
                                offs.ctypes.data_as(lp) if offsets else None, None)
    return int(rc), L.implisolid_last_error().decode(), offs


REFUSED = {
    "steps 0": (dict(steps=0), "implisolid_ray_spans: steps must be in [1, 65536]"),
    "steps 65537": (dict(steps=65537), "implisolid_ray_spans: steps must be in [1, 65536]"),
    "bisect -1": (dict(bisect=-1), "implisolid_ray_spans: bisect must be in [0, 32]"),
    "bisect 33": (dict(bisect=33), "implisolid_ray_spans: bisect must be in [0, 32]"),
    "empty range": (dict(t0=1.0, t1=1.0), "raycast: the range must be finite with t0 < t1"),
    "reversed range": (dict(t0=2.0, t1=1.0), "raycast: the range must be finite with t0 < t1"),
    "n -1": (dict(n=-1), "implisolid_ray_spans: n must be in [0, 2^24]"),
    "n 2^24 + 1": (dict(n=(1 << 24) + 1), "implisolid_ray_spans: n must be in [0, 2^24]"),
    "nan origin": (dict(o=(0, np.nan, 2)), "implisolid_ray_spans: every origin and direction must be finite"),
    "inf direction": (dict(d=(0, np.inf, -1)), "implisolid_ray_spans: every origin and direction must be finite"),
    "null shape": (dict(shape=None), "implisolid_ray_spans: bad arguments"),
    "null offsets": (dict(offsets=False), "implisolid_ray_spans: bad arguments"),
    "rawjscode": (dict(shape=json.dumps({"type": "rawjscode", "matrix": EYE}).encode()), None),
    "no rays, rawjscode": (dict(shape=json.dumps({"type": "rawjscode", "matrix": EYE}).encode(), n=0), None),
    "not json": (dict(shape=b'{"type": "iellipsoid", "matrix": [1, 0'), "JSON parse error: expected , or ]"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusal(impli, name):
    L = impli.lib()
    kw, msg = REFUSED[name]
    rc, got, _ = _call(L, **kw)
    assert rc == -1 and got and (msg is None or got == msg), got
    # a refused call leaves no result behind
    k, t = np.zeros(2, np.int32), np.zeros(2, f32)
    assert L.implisolid_ray_spans_copy(k.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), t.ctypes.data_as(fp), t.ctypes.data_as(fp), None) == -1
    assert impli.last_error() == "implisolid_ray_spans_copy: no spans to copy (the last implisolid_ray_spans failed, or none ran)"
    assert impli.ray_params(0, 1, 4).tolist() == [0, 0.25, 0.5, 0.75, 1] and impli.last_error() == "", "and the next host call works"


def test_no_rays_give_an_empty_result_without_a_device(impli):
    L = impli.lib()
    stats = np.full(8, 7, np.int64)
    offs = np.full(1, 7, np.int64)
    rc = L.implisolid_ray_spans(SPHERE, 0, None, None, 0, 0.5, 3.0, 64, 8, 0, offs.ctypes.data_as(lp), stats.ctypes.data_as(lp))
    assert rc == 0 and impli.last_error() == "" and offs.tolist() == [0] and stats.tolist() == [0] * 8
    assert L.implisolid_ray_spans_copy(None, None, None, None) == 0, "an empty result is a result"
    nrm = np.zeros(6, f32)
    assert L.implisolid_ray_spans_copy(None, None, None, nrm.ctypes.data_as(fp)) == -1, "normals the call did not compute"
    assert "no normals" in impli.last_error()
    offs, k, t, f, n, stats = impli.ray_spans(json.loads(SPHERE), np.zeros((0, 3)), np.zeros((0, 3)), 0.5, 3.0, 64, want_normals=True,
                                              return_stats=True)
    assert offs.tolist() == [0] and k.shape == (0, 2) and t.shape == f.shape == (0, 2) and n.shape == (0, 2, 3) and stats == [0] * 8
    with pytest.raises(impli.ImplisolidError):
        impli.ray_spans(json.loads(SPHERE), np.zeros((2, 3)), np.zeros((1, 3)), 0.5, 3.0, 64)


# ---- the restatement against analytic solids --------------------------------------------------------------------
def _ball(p, c, r):
    q = np.asarray(p, f32) - np.asarray(c, f32)
    return (f32(1) - (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]) / f32(r * r)).astype(f32)


def _sphere(p):
    return _ball(p, [0, 0, 0], 0.5)


def _two(p):
    return np.maximum(_ball(p, [0, 0, 0.5], 0.25), _ball(p, [0, 0, -0.5], 0.25))


def _shell(p):
    return np.minimum(_sphere(p), -_ball(p, [0, 0, 0], 0.25))


RANGE = (0.25, 3.0)
ULPS = 8 * float(np.spacing(f32(3.0)))   # p(t), its squares and their sum round a few times at magnitudes up to 3


def _within(t, want, step, B):
    """each end within step * 2^-B plus a few ulps of t1 of the analytic crossing, on the solid side"""
    t, want = np.asarray(t, np.float64), np.asarray(want, np.float64)
    slack = step * 2.0 ** -B + ULPS
    assert (t[:, 0] >= want[:, 0] - ULPS).all() and (t[:, 0] <= want[:, 0] + slack).all(), (t, want)
    assert (t[:, 1] <= want[:, 1] + ULPS).all() and (t[:, 1] >= want[:, 1] - slack).all(), (t, want)


@pytest.mark.parametrize("B", [0, 1, 20])
@pytest.mark.parametrize("N", [64, 65, 130])
def test_spans_of_analytic_solids(N, B):
    ts = np_raycast.params(RANGE[0], RANGE[1], N)
    step = (RANGE[1] - RANGE[0]) / N
    o = np.array([[0, 0, 2], [0, 0, 0]], f32)
    d = np.array([[0, 0, -1], [0, 0, 0]], f32)
    offs, k, t, f = np_rayspans.spans(_two, o, d, ts, B)
    assert offs.tolist() == [0, 2, 2] and k.dtype == np.int32 and t.dtype == f.dtype == np.float32
    _within(t, [[1.25, 1.75], [2.25, 2.75]], step, B)
    assert (~(f < 0)).all() and (k[:, 0] < k[:, 1]).all() and k[0, 1] < k[1, 0] and (t[:, 0] <= t[:, 1]).all()
    assert np.array_equal(f.view(np.uint32), _two(np_raycast.points(np.repeat(o[:1], 4, 0), np.repeat(d[:1], 4, 0), t.reshape(-1))).view(np.uint32).reshape(2, 2))
    # the first entry is raycast's hit
    hit, ht, hf = np_raycast.cast(_two, o, d, ts, B)
    assert hit[0] == k[0, 0] and ht[0] == t[0, 0] and hf[0] == f[0, 0] and hit[1] == -1
    offs, k, t, f = np_rayspans.spans(_shell, o, d, ts, B)
    assert offs.tolist() == [0, 2, 2], "two walls through the centre, none for a zero direction at the hollow centre"
    _within(t, [[1.5, 1.75], [2.25, 2.5]], step, B)
    if B == 0:
        assert np.array_equal(t[:, 0], ts[k[:, 0]]) and np.array_equal(t[:, 1], ts[k[:, 1] - 1])


def test_starts_inside_ends_inside_inside_throughout_and_misses():
    N, B = 65, 12
    ts = np_raycast.params(RANGE[0], 1.8, N)
    step = (1.8 - RANGE[0]) / N
    o = np.array([[0, 0, 0], [0, 0, 2], [0, 0, 0], [2, 2, 2], [0.1, 0, 0]], f32)
    d = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 0.1], [1, 0, 0], [0, 0, 0]], f32)
    offs, k, t, f = np_rayspans.spans(_sphere, o, d, ts, B)
    assert offs.tolist() == [0, 1, 2, 3, 3, 4]
    assert k[0, 0] == 0 and t[0, 0] == ts[0] and 1 <= k[0, 1] <= N and abs(float(t[0, 1]) - 0.5) <= step * 2.0 ** -B + ULPS, "starts inside"
    assert k[1].tolist()[1] == N + 1 and t[1, 1] == ts[N] and abs(float(t[1, 0]) - 1.5) <= step * 2.0 ** -B + ULPS, "ends inside"
    assert k[2].tolist() == [0, N + 1] and t[2].tolist() == [ts[0], ts[N]], "inside throughout"
    assert k[3].tolist() == [0, N + 1], "a zero direction inside"
    ends = np_raycast.points(o[[0, 1, 1, 2, 2]], d[[0, 1, 1, 2, 2]], np.array([t[0, 0], t[1, 0], t[1, 1], t[2, 0], t[2, 1]], f32))
    assert np.array_equal(np.array([f[0, 0], f[1, 0], f[1, 1], f[2, 0], f[2, 1]], f32).view(np.uint32), _sphere(ends).view(np.uint32))


def test_negative_zero_and_nan_samples_are_solid_and_a_span_may_hold_one_sample():
    vals = {0: np.array([-1, -0.0, -1, np.nan, -1], f32), 1: np.array([-0.0, -1, -1, -1, np.nan], f32), 2: np.full(5, -1, f32)}
    o = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], f32)
    d = np.array([[0, 1, 0]] * 3, f32)
    ts = np_raycast.params(0, 4, 4)

    def field(p):
        return np.array([vals[int(q[0])][int(round(float(q[1])))] for q in p], f32)
    offs, k, t, f = np_rayspans.spans(field, o, d, ts, 0)
    assert offs.tolist() == [0, 2, 4, 4]
    assert k.tolist() == [[1, 2], [3, 4], [0, 1], [4, 5]]
    assert t.tolist() == [[1, 1], [3, 3], [0, 0], [4, 4]], "B = 0: a single-sample span's ends coincide"
    assert f[0, 0] == 0 and np.signbit(f[0]).all() and np.isnan(f[1]).all() and np.signbit(f[2]).all() and np.isnan(f[3]).all()


def test_runs():
    s = np.array([[1, 1, 0, 1], [0, 0, 0, 0], [0, 1, 1, 1], [1, 0, 1, 0]], bool)
    rows, k_in, k_out = np_rayspans.runs(s)
    assert rows.tolist() == [0, 0, 2, 3, 3] and k_in.tolist() == [0, 3, 1, 0, 2] and k_out.tolist() == [2, 4, 4, 1, 3]


# ---- span_lengths ------------------------------------------------------------------------------------------------
def test_span_lengths(impli):
    offs = np.array([0, 2, 2, 3, 3], np.int64)
    t = np.array([[1, 2], [3, 3.5], [0, 4]], f32)
    d = np.array([[0, 0, 2], [1, 0, 0], [0, 3, 4], [1, 1, 1]], f32)
    length, count = impli.span_lengths(offs, t, d)
    assert length.dtype == np.float64 and count.dtype == np.int64
    assert length.tolist() == [3.0, 0.0, 20.0, 0.0] and count.tolist() == [2, 0, 1, 0]
    length, count = impli.span_lengths(np.zeros(1, np.int64), np.zeros((0, 2), f32), np.zeros((0, 3), f32))
    assert length.shape == count.shape == (0,)
    # float64 sums of float32 ends: no rounding to float32 in between
    t2 = np.array([[0.1, 0.7], [0.7, 3.3]], f32)
    length, _ = impli.span_lengths([0, 2], t2, [[0, 0, 1]])
    assert length[0] == (float(t2[0, 1]) - float(t2[0, 0])) + (float(t2[1, 1]) - float(t2[1, 0]))
    with pytest.raises(impli.ImplisolidError):
        impli.span_lengths(offs, t, d[:2])


# ---- the inputs of tests/test_gpu_rayspans.py ---------------------------------------------------------------------
ORACLE_NAMES = [n for n in inputs.NAMES if n != "sdf3d"]   # the sdf_3d field needs the library's evaluator


def test_the_new_solids_are_what_their_names_say(oracle):
    pts = np.array([[0, 0, 0.5], [0, 0, -0.5], [0, 0, 0], [0, 0, 0.8], [0.375, 0, 0], [0, 0.2, 0], [0.6, 0, 0]], f32)
    two = oracle.eval_implicit(oracle.mp5_to_nodes(json.dumps(inputs.TWO), False), pts)
    shell = oracle.eval_implicit(oracle.mp5_to_nodes(json.dumps(inputs.SHELL), False), pts)
    assert (two > 0).tolist() == [True, True, False, False, False, False, False]
    assert (shell > 0).tolist() == [False, False, False, False, True, False, False]
    assert np.abs(two - _two(pts)).max() < 1e-5 and np.abs(shell - _shell(pts)).max() < 1e-5


@pytest.mark.parametrize("name", ORACLE_NAMES)
def test_suite_rays_hold_no_one_and_several_spans(oracle, name):
    for N in (1, 64, 65, 130):
        rays = inputs.suite(None, oracle, name, N)
        assert len(rays) == inputs.N_RAYS
        offs, k, t, f, _ = inputs.reference(None, oracle, rays, 0, normals=False)
        count = np.diff(offs)
        print(name, N, "spans per ray: 0 x", int((count == 0).sum()), " 1 x", int((count == 1).sum()), " more x", int((count > 1).sum()))
        assert (count == 0).any() and (count == 1).any()
        assert count[0] >= 1 and k[offs[0], 0] == 0 and count[2] == 1 and k[offs[2]].tolist() == [0, N + 1], "starts inside"
        assert count[1] == 1 and k[offs[1]].tolist() == [N, N + 1], "ray 1 ends inside, on its last sample"
        assert count[3] == 0 and count[4] == 0
        if N >= 64 and name in inputs.SEVERAL:
            assert (count >= 2).sum() >= (2 if name in ("two", "shell") else 1), "several spans a ray"
        if N >= 64 and name in ("two", "shell"):
            first = len(rays) - len(inputs.EXTRA_O)
            assert count[first] == 2 and count[first + 3] == 0, "the axis ray crosses both; the hollow centre holds nothing"


@pytest.mark.parametrize("which", ["sphere", "two"])
def test_placed_entries_and_exits_fall_on_the_chosen_samples(oracle, which):
    rays = inputs.placed_case(which)
    N, ks = inputs.PLACED_N, inputs.PLACED_KS
    assert N == 4200 and inputs.nseg(N) == 66 and N % 64 != 0 and {64, 65, 4096, 4097, N} == set(ks)
    for B in (0, 24):
        offs, k, t, f, _ = inputs.reference(None, oracle, rays, B, normals=False)
        per = [k[offs[r]:offs[r + 1]] for r in range(len(rays))]
        for i, K in enumerate(ks):
            assert per[i][-1, 0] == K, "an entry at K"
            assert per[len(ks) + i][-1, 1] == K, "an exit at K"
        assert (~(f < 0)).all() and (t[:, 0] <= t[:, 1]).all()
    if which == "sphere":
        assert [len(p) for p in per] == [1] * len(rays)
        assert per[2].tolist() == [[4096, N + 1]] and per[3].tolist() == [[4097, N + 1]], "ends inside, across the batch boundary"
        assert per[4].tolist() == [[N, N + 1]] and per[5][0, 0] == 0 and per[6][0, 0] == 0, "the last sample alone; starts inside"
        assert per[10][0, 1] == inputs.ACROSS_K and 64 < per[10][0, 0] < 4096, "a span across the batch boundary that ends before N"
    else:
        assert [len(p) for p in per[2:5]] == [2, 2, 2] and [len(p) for p in per[7:10]] == [2, 2, 2], "the near sphere first"
        assert all(p[0, 1] < 4096 for p in per[2:4]) and per[2][1].tolist() == [4096, N + 1] and per[3][1].tolist() == [4097, N + 1]
        assert per[5][0, 0] == 0 and per[9][1, 1] == N and per[9][1, 0] > 64 * 57, "an exit on the last sample"
