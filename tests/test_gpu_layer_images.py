"""What the seven layer queries share on the host (abi_layers.hip LayerImages, abi_common.hpp StagingSlots and
CarriedLayer): the chunk walk, the scratch, the staging slots and the carried layers.  Their own suites compare
each with its restatement; here the seven run on one engine, alone with one chunk and then interleaved with a layer
per chunk, and every integer must be the same.  40 x 40 pixels are 3 x 3 raster tiles with an image pitch (48) that
is not the width, so raster's pitched copy runs; five chunks use both staging slots of raster, supports and runs and
end on the first; islands, distance and supports carry a layer from each chunk to the next; bodies grows its
stack-wide arrays chunk by chunk.  The hollow wall has reach 1: its rings hold min(1 + 2 reach, 5) = 3 layers,
fewer than the call, and wrap.  On Z5 the restatements in tests/ give, at these settings: 4 core voxels (hollow,
threshold 1, wall2 {1, 0}, ends 0), 8 tips in layers 1, 2 and 3 (supports, threshold 3, reach2 2, cell 5: layers 2
and 3 lie on a layer that was itself carried onto), 77 runs in 5 layers, 6 bodies.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_raster as gr   # noqa: E402  (its shapes, rects and planes; its tests are not collected from here)

pytestmark = pytest.mark.gpu

Z5 = np.array([-0.3, -0.125, 0.05, -0.2, -0.55], np.float32)
CHUNK_VARS = ("IMPLISOLID_RASTER_CHUNK", "IMPLISOLID_ISLANDS_CHUNK", "IMPLISOLID_DISTANCE_CHUNK", "IMPLISOLID_HOLLOW_CHUNK",
              "IMPLISOLID_SUPPORTS_CHUNK", "IMPLISOLID_RUNS_CHUNK", "IMPLISOLID_BODIES_CHUNK")
WALL2 = np.array([1, 0], np.int64)   # reach 1


def _same(got, want):
    """every array of a result equal, integer for integer; structured arrays field by field"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


@pytest.mark.parametrize("level", [0, 2])
def test_interleaved_and_chunked_calls_equal_the_solo_ones(impli, level, monkeypatch):
    a = (gr.SHAPES["tree_deep"], gr.RECTS["non_dyadic"], 40, 40, Z5)
    other = (gr.SHAPES["tree_deep"], gr.RECTS["non_dyadic"], 33, 17, gr.Z)
    impli.set_pruning(level)
    try:
        cov, sums, rstats = impli.raster_layers(*a, 2, return_stats=True)
        offs, comps, labels, istats = impli.layer_islands(*a, 2, 3, 8, want_labels=True, return_stats=True)
        dist, rec, dstats = impli.layer_distance(*a, 2, 3, 2, return_stats=True)
        *hollow, hstats = impli.layer_hollow(*a, WALL2, 2, 1, 0, return_stats=True)
        *tips, sstats = impli.layer_supports(*a, 5, 2, 3, 2, return_stats=True)
        *runs, nstats = impli.layer_runs(*a, 2, 3, return_stats=True)
        *bodies, bstats = impli.layer_bodies(*a, 2, 3, want_runs=True, return_stats=True)
        for v in CHUNK_VARS:
            monkeypatch.setenv(v, "1")   # below one layer's tiles: a layer per chunk
        dist_ms = impli.layer_distance_kernel_ms(False)
        dist2, rec2, dstats2 = impli.layer_distance(*a, 2, 3, 2, return_stats=True)
        *tips2, sstats2 = impli.layer_supports(*a, 5, 2, 3, 2, return_stats=True)
        impli.islands_kernel_ms(True)
        try:
            offs2, comps2, labels2, istats2 = impli.layer_islands(*a, 2, 3, 8, want_labels=True, return_stats=True)
        finally:
            ms = impli.islands_kernel_ms(False)
        impli.layer_islands(*other, 4, 5, 4, want_labels=True)   # another size: the scratch is resized and used again
        *hollow2, hstats2 = impli.layer_hollow(*a, WALL2, 2, 1, 0, return_stats=True)
        impli.layer_distance(*other, 4, 5, 0)
        impli.layer_runs(*other, 4, 5)
        *bodies2, bstats2 = impli.layer_bodies(*a, 2, 3, want_runs=True, return_stats=True)
        impli.layer_supports(*other, 3, 4, 5, 0)
        *runs2, nstats2 = impli.layer_runs(*a, 2, 3, return_stats=True)
        impli.layer_hollow(*other, WALL2, 4, 5, 3)
        impli.layer_bodies(*other, 4, 5)
        cov2, sums2, rstats2 = impli.raster_layers(*a, 2, return_stats=True)
    finally:
        impli.set_pruning(2)
    print("raster, tiles, merge, rows + scan, records + tally ms over five chunks", ms)
    assert len(ms) == 5 and all(v >= 0 for v in ms)
    assert impli.islands_kernel_ms(False) == ms, "an untimed call leaves the last timed call's figures"
    assert impli.layer_distance_kernel_ms(False) == dist_ms
    assert rstats[4] == istats[4] == dstats[4] == 1 and rstats2[4] == istats2[4] == dstats2[4] == 5
    assert np.array_equal(cov2, cov) and np.array_equal(sums2, sums) and rstats2[:4] == rstats[:4]
    assert np.array_equal(offs2, offs) and np.array_equal(comps2, comps) and np.array_equal(labels2, labels)
    assert istats2[:4] == istats[:4] and istats2[5:] == istats[5:]
    assert np.array_equal(dist2, dist) and np.array_equal(rec2, rec) and dstats2[:4] == dstats[:4] and dstats2[5:] == dstats[5:]
    assert rstats[:4] == istats[:4] == dstats[:4], "one image head"
    assert sums.sum() > 0 and istats[7] > 0 and len(comps) > 0 and dstats[5] > 0 and (dist > 0).any(), "or nothing was compared"
    assert cov.shape == (5, 40, 40) and labels.shape == dist.shape == (5, 40, 40)
    # hollow, supports, runs and bodies by the same scheme
    for name, one, many, st1, st5 in (("hollow", hollow, hollow2, hstats, hstats2), ("supports", tips, tips2, sstats, sstats2),
                                      ("runs", runs, runs2, nstats, nstats2), ("bodies", bodies, bodies2, bstats, bstats2)):
        print(name, "stats", st1, st5)
        _same(many, one)
        assert st1[4] == 1 and st5[4] == 5, name
        assert st5[:4] == st1[:4] and st5[5:] == st1[5:], name
    # hollow at threshold 1 and bodies' and runs' heads at threshold 3 rasterise the same image: the head knows no threshold
    assert rstats[:4] == hstats[:4] == sstats[:4] == nstats[:4] == bstats[:4], "one image head"
    out, hrec = hollow
    assert out.shape == (5, 40, 40) and hstats[6] > 0 and (out[cov > 0] == 0).any(), "core voxels, or nothing was compared"
    assert hstats[7] == hstats2[7] == 5, "every layer is transformed once, in one chunk or in five"
    tip_rows, tip_offs, _ = tips
    assert len(tip_rows) > 0 and tip_offs[-1] > tip_offs[2], "tips above a layer that was itself carried onto, or nothing was compared"
    run_offs, start, value, run_sums = runs
    assert len(start) > 5 and np.array_equal(run_sums, sums), "more runs than layers, or nothing was compared"
    body_offs, body_rec, body_runs = bodies
    assert len(body_rec) >= 1 and len(body_runs) == body_offs[-1] > 0, "or nothing was compared"
