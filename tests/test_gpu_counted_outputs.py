"""What slice_layers, layer_islands, layer_runs and ray_spans share on the host (abi_common.hpp CountedOutput,
ResultSlot, PassTimer): per-item counts, their scan, the read-back of the chunk's group offsets, the running
total and the result slot.  Their own suites compare each with its restatement; here the four run on one
engine, alone with one chunk and then interleaved with one group (a layer, a ray) per chunk, and every integer
and every float's bits must be the same.  40 x 40 pixels are 3 x 3 raster tiles with an image pitch (48) that
is not the width; a slice resolution of 40 gives 3 x 3 slice tiles; 130 steps are three ray segments.  The
middle plane lies off the solid and some rays in the middle miss it, so a chunk that produces nothing sits
between chunks that do: the first test asserts that of the inputs without a GPU.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_raster    # noqa: E402
import np_raycast   # noqa: E402
import np_rayspans  # noqa: E402
import np_restate   # noqa: E402
import np_runs      # noqa: E402
import np_slice     # noqa: E402
import test_gpu_raster as gr   # noqa: E402  (its shapes, rects and planes; its tests are not collected from here)

SHAPE, RECT = gr.SHAPES["tree_deep"], gr.RECTS["non_dyadic"]
Z5 = np.array([-0.3, -0.125, 3.0, 0.05, -0.2], np.float32)   # the third plane lies off the solid
W = H = R = 40
SS = 2
T0, T1, STEPS, BISECT = 0.25, 3.5, 130, 8
CHUNK_VARS = ("IMPLISOLID_SLICE_CHUNK", "IMPLISOLID_ISLANDS_CHUNK", "IMPLISOLID_RUNS_CHUNK", "IMPLISOLID_SPAN_CHUNK")


def _rays():
    """a 10 x 10 grid of rays down the z axis from z = 2, row by row: each row starts and ends beside the solid"""
    x, y = np.meshgrid(np.linspace(-0.9, 1.2, 10), np.linspace(-1.0, 0.8, 10))
    o = np.stack([x.ravel(), y.ravel(), np.full(100, 2.0)], -1).astype(np.float32)
    return o, np.tile(np.array([0, 0, -1], np.float32), (100, 1))


def _field(pts):
    return np.asarray(np_restate.evaluate(SHAPE, *np.asarray(pts, np.float32).T), np.float32)


def _an_empty_one_between_full_ones(count):
    count = np.asarray(count)
    return any(count[i] == 0 and count[:i].any() and count[i + 1:].any() for i in range(1, len(count) - 1))


def test_the_inputs_hold_a_chunk_without_a_record_between_chunks_with_records():
    # on the restatements alone: the third plane holds no solid sample (no segment, no component, one run) and the
    # others hold some; rays in the middle of the list miss the solid, with rays that hit it before and behind
    F = _field(np_raster.points(*np_raster.coords(RECT, W, H, SS), Z5)).reshape(5, H * SS, W * SS)
    cov = np_raster.coverage(F, SS)[0]
    assert not cov[2].any() and all(cov[l].any() for l in (0, 1, 3, 4))
    assert np.diff(np_runs.encode(cov, 0)[0]).tolist()[2] == 1 and _an_empty_one_between_full_ones(np.diff(np_runs.encode(cov, 0)[0]) - 1)
    xs, ys = np_slice.coords(np.asarray(RECT, np.float32), R)
    G = _field(np_slice.points(xs, ys, Z5)).reshape(5, R + 1, R + 1)
    assert _an_empty_one_between_full_ones(np.diff(np_slice.march(G, xs, ys)[2])) and (G[2] < 0).all()
    o, d = _rays()
    count = np.diff(np_rayspans.spans(_field, o, d, np_raycast.params(T0, T1, STEPS), BISECT)[0])
    assert _an_empty_one_between_full_ones(count) and (count > 1).any(), "and a ray of several spans"


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 2])
def test_interleaved_and_chunked_calls_equal_the_solo_ones(impli, level, monkeypatch):
    a = (SHAPE, RECT, W, H, Z5, SS)
    other = (SHAPE, RECT, 33, 17, gr.Z, 4)
    o, d = _rays()
    rays = (SHAPE, o, d, T0, T1, STEPS, BISECT)
    impli.set_pruning(level)
    try:
        seg, keys, soffs, sstats = impli.slice_layers(SHAPE, RECT, R, Z5, return_stats=True)
        ioffs, comps, labels, istats = impli.layer_islands(*a, 3, 8, want_labels=True, return_stats=True)
        roffs, start, value, sums, rstats = impli.layer_runs(*a, 0, return_stats=True)
        poffs, k, t, f, nrm, pstats = impli.ray_spans(*rays, want_normals=True, return_stats=True)
        off_solid = impli.slice_layers(SHAPE, RECT, R, Z5[2:3], return_stats=True)[3]
        for v in CHUNK_VARS:
            monkeypatch.setenv(v, "1")   # below one layer's tiles: a layer per chunk; a ray per chunk
        impli.layer_runs_kernel_ms(True)
        impli.ray_spans_kernel_ms(True)
        try:
            poffs2, k2, t2, f2, nrm2, pstats2 = impli.ray_spans(*rays, want_normals=True, return_stats=True)
            ioffs2, comps2, labels2, istats2 = impli.layer_islands(*a, 3, 8, want_labels=True, return_stats=True)
            impli.layer_runs(*other, 5)   # another size: the scan's buffer is resized and carved again
            impli.slice_layers(SHAPE, RECT, 24, gr.Z)
            roffs2, start2, value2, sums2, rstats2 = impli.layer_runs(*a, 0, return_stats=True)
        finally:
            run_ms = impli.layer_runs_kernel_ms(False)
            span_ms = impli.ray_spans_kernel_ms(False)
        impli.layer_islands(*other, 5, 4)
        impli.ray_spans(SHAPE, o[:7], d[:7], T0, T1, 64, 0)
        seg2, keys2, soffs2, sstats2 = impli.slice_layers(SHAPE, RECT, R, Z5, return_stats=True)
        untimed = impli.layer_runs(*a, 0, return_stats=True)
    finally:
        impli.set_pruning(2)
    print("runs: raster, count + scan, emit ms over five chunks", run_ms, "spans: march, scan + tally + emit, refine ms", span_ms)
    assert len(run_ms) == 3 and all(v >= 0 for v in run_ms) and len(span_ms) == 3 and all(v >= 0 for v in span_ms)
    assert impli.layer_runs_kernel_ms(False) == run_ms, "an untimed call leaves the last timed call's figures"
    assert impli.ray_spans_kernel_ms(False) == span_ms
    assert sstats[3] == istats[4] == rstats[4] == pstats[7] == 1
    assert sstats2[3] == istats2[4] == rstats2[4] == 5 and pstats2[7] == len(o)
    # a chunk without a record between chunks with records, in every query
    assert _an_empty_one_between_full_ones(np.diff(soffs)) and np.diff(soffs)[2] == 0
    assert level == 0 or off_solid[1] == 0, "pruning lists no tile of the plane off the solid: no scan for that chunk"
    assert _an_empty_one_between_full_ones(np.diff(ioffs)) and np.diff(ioffs)[2] == 0
    assert np.diff(roffs)[2] == 1 and (np.diff(roffs)[[0, 1, 3, 4]] > 1).all()
    assert _an_empty_one_between_full_ones(np.diff(poffs))
    # the chunked and interleaved calls against the solo ones
    assert np.array_equal(soffs2, soffs) and np.array_equal(keys2, keys) and np.array_equal(_u32(seg2), _u32(seg))
    assert seg2.shape == seg.shape and sstats2[:3] == sstats[:3]
    assert np.array_equal(ioffs2, ioffs) and np.array_equal(comps2, comps) and np.array_equal(labels2, labels)
    assert istats2[:4] == istats[:4] and istats2[5:] == istats[5:]
    assert np.array_equal(roffs2, roffs) and np.array_equal(start2, start) and np.array_equal(value2, value)
    assert np.array_equal(sums2, sums) and rstats2[:4] == rstats[:4] and rstats2[5:] == rstats[5:]
    assert all(np.array_equal(x, y) for x, y in zip(untimed[:4], (roffs, start, value, sums))), "timed or not, the same result"
    assert np.array_equal(poffs2, poffs) and np.array_equal(k2, k) and pstats2[:7] == pstats[:7]
    assert np.array_equal(_u32(t2), _u32(t)) and np.array_equal(_u32(f2), _u32(f)) and np.array_equal(_u32(nrm2), _u32(nrm))
    assert len(seg) > 0 and len(comps) > 0 and len(start) > 5 and len(k) > 0 and labels.shape == (5, H, W), "or nothing was compared"
